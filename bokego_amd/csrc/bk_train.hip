// bk_train.hip -- training kernels of the 9x9 trunk (include/bokego_train.h): implicit-GEMM convolutions (forward,
// input gradient, weight gradient) on fp32 MFMA, train/eval BatchNorm2d + ReLU with their gradients, and the move
// sampler of the REINFORCE playouts.  Stateless: the caller owns every buffer and the stream.  Nothing here uses float
// atomics, so every result is a fixed-order sum.
#include <hip/hip_runtime.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int P = 81;                 // points of the board
constexpr int BM = BKT_COUT;          // output channels: one GEMM tile spans all of them
constexpr int BN = 64;                // GEMM columns per workgroup
constexpr int BK = 16;                // reduction depth per LDS stage
constexpr int PAD = 16;               // LDS row padding: the four k-rows of one MFMA operand read land in different banks
constexpr int NT = 256;               // four waves: a 2x2 grid of 64x32 wave tiles
constexpr int RT = 256;               // threads of the per-channel reductions
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// One BK-deep stage of the 128 x 64 workgroup tile: wave w owns rows (w & 1) * 64 .. +64, columns (w >> 1) * 32 .. +32,
// as 4 x 2 tiles of 16 x 16.  16x16x4 f32 MFMA operands: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15].
__device__ __forceinline__ void mma_stage(const float (*As)[BM + PAD], const float (*Bs)[BN + PAD], f32x4 (&acc)[4][2],
                                          int lane, int wm, int wn) {
    const int c = lane & 15;
#pragma unroll
    for (int kq = 0; kq < BK; kq += 4) {
        const int kr = kq + (lane >> 4);
        float a[4], b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = As[kr][wm + 16 * i + c];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Bs[kr][wn + 16 * j + c];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

// A stage's 16-deep products go into fresh accumulators, which are then added to the running sums with Kahan
// compensation: a dot product of K = 1152 carries the rounding of a 16-term MFMA chain plus O(eps^2), not of a
// 1152-term chain.  This matters where a gradient is a small difference of large partial sums (measured: 5e-4 relative
// error of the deep layers' gradients in the value net with plain chains).  A running sum that reaches +-Inf
// becomes NaN at the next stage ((t - acc) - y is inf - inf): the allowance of bokego_train.h's "Non-finite values".
__device__ __forceinline__ void stage_into(const float (*As)[BM + PAD], const float (*Bs)[BN + PAD], f32x4 (&acc)[4][2],
                                           f32x4 (&comp)[4][2], int lane, int wm, int wn) {
    f32x4 part[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) part[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    mma_stage(As, Bs, part, lane, wm, wn);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 y = part[i][j] - comp[i][j];
            const f32x4 t = acc[i][j] + y;
            comp[i][j] = (t - acc[i][j]) - y;
            acc[i][j] = t;
        }
}

// ---- forward: y[b][m][p] = sum_k wt[k][m] * im2col(x)[k][b*81 + p] (+ bias[m]) ----------------------------------------
// Also the input gradient (wt = the rotated, channel-swapped filters, x = dy, no bias).
// SAN (the input gradient): a weight that is not finite enters the GEMM as 0 and is added by dgrad_nonfinite_kernel, over
// the taps that lie on the board only -- the GEMM would multiply it with the zero a tap off the board reads.
template <int KS, bool SAN = false>
__global__ __launch_bounds__(NT) void conv_fwd_kernel(const float *__restrict__ x, const float *__restrict__ wt,
                                                      const float *__restrict__ bias, float *__restrict__ y, int batch,
                                                      int cin) {
    __shared__ float As[BK][BM + PAD];
    __shared__ float Bs[BK][BN + PAD];
    constexpr int KK = KS * KS, H = KS / 2;
    const int K = cin * KK, N = batch * P;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n0 = blockIdx.x * BN;
    // A (weights, K-major): this thread loads row am of k-rows ak, ak + 2, ...; B (gathered input): column bn of
    // k-rows bk, bk + 4, ...  Both are coalesced along the lanes.
    const int am = t & (BM - 1), ak = t >> 7;
    const int bn = t & (BN - 1), bk = t >> 6;
    const int n = n0 + bn;
    const bool nvalid = n < N;
    const int b = nvalid ? n / P : 0, p = nvalid ? n - (n / P) * P : 0;
    const int py = p / 9, px = p - (p / 9) * 9;
    const float *xb = x + (size_t)b * cin * P;

    float ra[8], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = k0 + ak + 2 * i;
            ra[i] = kk < K ? wt[(size_t)kk * BM + am] : 0.f;
            if (SAN && not_finite(ra[i])) ra[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = k0 + bk + 4 * i;
            float v = 0.f;
            if (nvalid && kk < K) {
                const int ci = kk / KK, tap = kk - ci * KK;
                const int yy = py + tap / KS - H, xx = px + (tap - (tap / KS) * KS) - H;
                if ((unsigned)yy < 9u && (unsigned)xx < 9u) v = xb[ci * P + yy * 9 + xx];
            }
            rb[i] = v;
        }
    };

    f32x4 acc[4][2], comp[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = comp[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (w & 1) * 64, wn = (w >> 1) * 32;

    load(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) As[ak + 2 * i][am] = ra[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[bk + 4 * i][bn] = rb[i];
        __syncthreads();
        if (k0 + BK < K) load(k0 + BK);  // the next stage's global loads overlap this stage's MFMAs
        stage_into(As, Bs, acc, comp, lane, wm, wn);
        __syncthreads();
    }

    // C/D of 16x16x4: lane l, register r -> row (l >> 4) * 4 + r, column l & 15
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nn = n0 + wn + 16 * j + (lane & 15);
        if (nn >= N) continue;
        const int ob = nn / P, op = nn - ob * P;
        float *yb = y + (size_t)ob * BM * P + op;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = wm + 16 * i + (lane >> 4) * 4 + r;
                yb[m * P] = acc[i][j][r] + (bias ? bias[m] : 0.f);
            }
    }
}

// The input gradient's weights that are not finite (conv_fwd_kernel<3, true> took them as 0): workgroup m adds
// w * dy[b][co][p + tap] to dx[b][m][p] for each of them, over the taps on the board -- the terms of the float64 input gradient,
// no others.  With finite weights it reads the 1152 weights of its channel and returns.  One thread owns an element of dx.
__global__ __launch_bounds__(256) void dgrad_nonfinite_kernel(const float *__restrict__ dy, const float *__restrict__ wt,
                                                              float *__restrict__ dx, int batch) {
    const int m = blockIdx.x, t = threadIdx.x;
    int any = 0;
    for (int k = t; k < BM * 9; k += 256) any |= not_finite(wt[(size_t)k * BM + m]);
    if (!__syncthreads_or(any)) return;
    for (int i = t; i < batch * P; i += 256) {
        const int b = i / P, p = i - b * P, py = p / 9, px = p - (p / 9) * 9;
        float s = 0.f;
        bool hit = false;
        for (int k = 0; k < BM * 9; ++k) {
            const float w = wt[(size_t)k * BM + m];
            if (!not_finite(w)) continue;
            const int co = k / 9, tap = k - co * 9;
            const int yy = py + tap / 3 - 1, xx = px + (tap - (tap / 3) * 3) - 1;
            if ((unsigned)yy < 9u && (unsigned)xx < 9u) {
                s += w * dy[((size_t)b * BM + co) * P + yy * 9 + xx];
                hit = true;
            }
        }
        if (hit) dx[((size_t)b * BM + m) * P + p] += s;
    }
}

// ---- weight gradient: part[chunk][m][n] = sum over the chunk's (b, p) of dy[b][m][p] * im2col(x)[n][b*81 + p] ----------
template <int KS>
__global__ __launch_bounds__(NT) void conv_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                        float *__restrict__ part, int batch, int cin) {
    __shared__ float As[BK][BM + PAD];
    __shared__ float Bs[BK][BN + PAD];
    constexpr int KK = KS * KS, H = KS / 2;
    const int NC = cin * KK;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n0 = blockIdx.x * BN, chunk = blockIdx.y;
    const int b_end = min(batch, (chunk + 1) * BKT_WGRAD_CHUNK);
    const int K0 = chunk * BKT_WGRAD_CHUNK * P, K1 = b_end * P;
    // both operands: k-row kr = t & 15 (consecutive lanes walk consecutive points), rows / columns (t >> 4) + 16 i
    const int kr = t & 15, r0 = t >> 4;
    int coff[4], cy[4], cx[4];
    bool cval[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int nn = n0 + r0 + 16 * i;
        cval[i] = nn < NC;
        const int ci = cval[i] ? nn / KK : 0, tap = cval[i] ? nn - (nn / KK) * KK : 0;
        coff[i] = ci * P;
        cy[i] = tap / KS - H;
        cx[i] = tap - (tap / KS) * KS - H;
    }

    float ra[8], rb[4];
    auto load = [&](int k0) {
        const int k = k0 + kr;
        const bool kv = k < K1;
        const int b = kv ? k / P : 0, p = kv ? k - (k / P) * P : 0;
        const int py = p / 9, px = p - (p / 9) * 9;
        const float *dyb = dy + (size_t)b * BM * P + p;
        const float *xb = x + (size_t)b * cin * P;
#pragma unroll
        for (int i = 0; i < 8; ++i) ra[i] = kv ? dyb[(r0 + 16 * i) * P] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int yy = py + cy[i], xx = px + cx[i];
            rb[i] = (kv && cval[i] && (unsigned)yy < 9u && (unsigned)xx < 9u) ? xb[coff[i] + yy * 9 + xx] : 0.f;
        }
    };

    f32x4 acc[4][2], comp[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = comp[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (w & 1) * 64, wn = (w >> 1) * 32;

    load(K0);
    for (int k0 = K0; k0 < K1; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) As[kr][r0 + 16 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[kr][r0 + 16 * i] = rb[i];
        __syncthreads();
        if (k0 + BK < K1) load(k0 + BK);
        stage_into(As, Bs, acc, comp, lane, wm, wn);
        __syncthreads();
    }

    float *pc = part + (size_t)chunk * BM * NC;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nn = n0 + wn + 16 * j + (lane & 15);
        if (nn >= NC) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) pc[(size_t)(wm + 16 * i + (lane >> 4) * 4 + r) * NC + nn] = acc[i][j][r];
    }
}

// dw[i] = sum over chunks, in chunk order, of part[chunk][i]
__global__ __launch_bounds__(256) void chunk_sum_kernel(const float *__restrict__ part, float *__restrict__ dw, int n,
                                                        int chunks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * n + i];
    dw[i] = s;
}

__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ w, float *__restrict__ wt, int K) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // i = k * 128 + m
    if (i >= K * BM) return;
    const int k = i / BM, m = i - k * BM;
    wt[i] = w[(size_t)m * K + k];
}

// wt[(co * 9 + tap) * 128 + ci] = w[co][ci][8 - tap]: the 3x3 filters turned by 180 degrees, input and output swapped
__global__ __launch_bounds__(256) void pack_dgrad_kernel(const float *__restrict__ w, float *__restrict__ wt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BM * BM * 9) return;
    const int ci = i % BM, k = i / BM, co = k / 9, tap = k - co * 9;
    wt[i] = w[((size_t)co * BM + ci) * 9 + (8 - tap)];
}

// ---- per-channel reductions over B*81 values, in two fixed-order steps: workgroup (c, s) sums slice s (boards
// 16 s .. 16 s + 15) of channel c -- a thread's strided serial sum, then an LDS tree -- into part[s][c]; a finalize kernel adds
// the slices of a channel in slice order.  Sums are kept in double: they feed every element of the BatchNorm outputs.
__device__ __forceinline__ void tree_sum2(double &a, double &b, double (*sh)[RT]) {
    const int t = threadIdx.x;
    sh[0][t] = a;
    sh[1][t] = b;
    __syncthreads();
#pragma unroll
    for (int s = RT / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] += sh[0][t + s];
            sh[1][t] += sh[1][t + s];
        }
        __syncthreads();
    }
    a = sh[0][0];
    b = sh[1][0];
}

// Non-finite values pass through (bokego_train.h, "Non-finite values"): fmaxf(v, 0) and `y > 0 ? dy : 0` would turn a NaN
// into 0, so the ReLU and its mask are written with the one comparison that is false for a NaN.
__device__ __forceinline__ float relu_keep_nan(float v) { return v <= 0.f ? 0.f : v; }
__device__ __forceinline__ float relu_mask(float y, float dy) { return y <= 0.f ? 0.f : dy; }
// (xc) * invstd * gamma + beta with xc = x - mean.  An infinite gamma takes float64 torch's form of the same expression,
// x * a + (beta - mean * a) with a = invstd * gamma, whose Inf - Inf marks the element NaN where x and the mean have one sign:
// the set the "Non-finite values" rule of bokego_train.h is stated against.  A finite gamma never takes that branch.
__device__ __forceinline__ float bn_affine(float x, float mean, float invstd, float gamma, float beta) {
    if ((__float_as_uint(gamma) & 0x7FFFFFFFu) == 0x7F800000u) {
        const float a = invstd * gamma;
        return x * a + (beta - mean * a);
    }
    return (x - mean) * invstd * gamma + beta;
}

enum { SUM_X_XX = 0, SUM_DZ_DZXHAT = 1, SUM_DY = 2 };

// part[(s * C + c) * 2 + {0, 1}]:  SUM_X_XX: sum x, sum x^2;  SUM_DZ_DZXHAT: sum dz, sum dz * xhat (dz = dy where y > 0);
// SUM_DY: sum dy
template <int MODE>
__global__ __launch_bounds__(RT) void chan_partial_kernel(const float *__restrict__ a, const float *__restrict__ y,
                                                          const float *__restrict__ x, const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, double *__restrict__ part,
                                                          int batch, int C) {
    __shared__ double sh[2][RT];
    const int c = blockIdx.x, s = blockIdx.y;
    const int b0 = s * BKT_WGRAD_CHUNK, nb = min(batch - b0, BKT_WGRAD_CHUNK);
    float mu = 0.f, is = 0.f;
    if (MODE == SUM_DZ_DZXHAT) {
        mu = mean[c];
        is = invstd[c];
    }
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nb * P; i += RT) {
        const int b = b0 + i / P;
        const size_t j = ((size_t)b * C + c) * P + (i - (i / P) * P);
        if (MODE == SUM_X_XX) {
            const double v = a[j];
            s0 += v;
            s1 += v * v;
        } else if (MODE == SUM_DZ_DZXHAT) {
            const float dz = relu_mask(y[j], a[j]);
            s0 += dz;
            s1 += (double)dz * (double)((x[j] - mu) * is);
        } else {
            s0 += a[j];
        }
    }
    tree_sum2(s0, s1, sh);
    if (threadIdx.x == 0) {
        part[((size_t)s * C + c) * 2] = s0;
        part[((size_t)s * C + c) * 2 + 1] = s1;
    }
}

__device__ __forceinline__ void slice_sums(const double *__restrict__ part, int slices, int C, int c, double &s0,
                                           double &s1) {
    s0 = s1 = 0.0;
    for (int s = 0; s < slices; ++s) {
        s0 += part[((size_t)s * C + c) * 2];
        s1 += part[((size_t)s * C + c) * 2 + 1];
    }
}

// mean, biased variance, inverse std, running statistics (torch's update: unbiased variance into running_var)
__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const double *__restrict__ part, int slices,
                                                                float *running_mean, float *running_var, int64_t *nbt,
                                                                float momentum, float eps,
                                                                float *__restrict__ save_mean,
                                                                float *__restrict__ save_invstd, int batch, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    double s0, s1;
    slice_sums(part, slices, C, c, s0, s1);
    const double n = (double)batch * P;
    const double mean = s0 / n;
    double var = s1 / n - mean * mean;
    if (var < 0.0) var = 0.0;  // rounding only; a NaN (one Inf in the channel: inf - inf) stays a NaN
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * (var * n / (n - 1.0)));
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double *__restrict__ part, int slices,
                                                              float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                              int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0, s1;
    slice_sums(part, slices, C, c, s0, s1);
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
}

__global__ __launch_bounds__(256) void chan_sum_finalize_kernel(const double *__restrict__ part, int slices,
                                                                float *__restrict__ out, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0, s1;
    slice_sums(part, slices, C, c, s0, s1);
    out[c] = (float)s0;
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ x, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, float *__restrict__ y,
                                                       size_t total, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / P) % C);
    y[i] = relu_keep_nan(bn_affine(x[i], mean[c], invstd[c], gamma[c], beta[c]));
}

__global__ __launch_bounds__(256) void bn_eval_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, const float *__restrict__ rmean,
                                                      const float *__restrict__ rvar, float eps, float *__restrict__ y,
                                                      size_t total, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / P) % C);
    y[i] = relu_keep_nan(bn_affine(x[i], rmean[c], 1.f / sqrtf(rvar[c] + eps), gamma[c], beta[c]));
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                           const float *__restrict__ x, const float *__restrict__ gamma,
                                                           const float *__restrict__ mean,
                                                           const float *__restrict__ invstd,
                                                           const float *__restrict__ dgamma,
                                                           const float *__restrict__ dbeta, float *__restrict__ dx,
                                                           size_t total, int C, float inv_n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / P) % C);
    const float is = invstd[c];
    const float dz = relu_mask(y[i], dy[i]);
    const float xhat = (x[i] - mean[c]) * is;
    dx[i] = gamma[c] * is * (dz - dbeta[c] * inv_n - xhat * (dgamma[c] * inv_n));
}

// Eval-mode (frozen statistics) analogue of chan_partial_kernel<SUM_DZ_DZXHAT>: part[(s * C + c) * 2 + {0, 1}] = sum dz,
// sum dz * (x - running_mean) * invstd over slice s, dz = dy where y > 0, invstd = 1/sqrt(running_var + eps) in double.
__global__ __launch_bounds__(RT) void bn_eval_bwd_partial_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                                 const float *__restrict__ x,
                                                                 const float *__restrict__ rmean,
                                                                 const float *__restrict__ rvar, float eps,
                                                                 double *__restrict__ part, int batch, int C) {
    __shared__ double sh[2][RT];
    const int c = blockIdx.x, s = blockIdx.y;
    const int b0 = s * BKT_WGRAD_CHUNK, nb = min(batch - b0, BKT_WGRAD_CHUNK);
    const double mu = rmean[c], is = 1.0 / sqrt((double)rvar[c] + (double)eps);
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nb * P; i += RT) {
        const int b = b0 + i / P;
        const size_t j = ((size_t)b * C + c) * P + (i - (i / P) * P);
        const float dz = relu_mask(y[j], dy[j]);
        s0 += dz;
        s1 += (double)dz * (((double)x[j] - mu) * is);
    }
    tree_sum2(s0, s1, sh);
    if (threadIdx.x == 0) {
        part[((size_t)s * C + c) * 2] = s0;
        part[((size_t)s * C + c) * 2 + 1] = s1;
    }
}

// dx = dy * [y > 0] * gamma / sqrt(running_var + eps): the scale bn_eval_kernel applies, in the same fp32 form
__global__ __launch_bounds__(256) void bn_eval_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ rvar, float eps,
                                                                float *__restrict__ dx, size_t total, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / P) % C);
    const float dz = relu_mask(y[i], dy[i]);
    dx[i] = dz * (gamma[c] * (1.f / sqrtf(rvar[c] + eps)));
}

// ---- move sampling: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) and one wave64 per row ---------------
constexpr int SAMPLE_WAVES = 4;       // rows per workgroup
constexpr int LEGAL_PLANE = 5;        // nnet.features' "legal" plane: bkt_sample_moves' mask, with a row stride of 27 planes

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
    }
}

// The bit tests of the degenerate-row contract (bokego_train.h): integer logic, which no float comparison can defeat.
__device__ __forceinline__ bool is_nan_bits(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) > 0x7F800000u; }
__device__ __forceinline__ bool is_nan_or_pinf(float v) { return is_nan_bits(v) || __float_as_uint(v) == 0x7F800000u; }

// Lane l holds points l and 64 + l (the second only for l < 17).  Every branch below is uniform over the wave.
// mask[row * mask_stride + i] != 0: point i may be played (bkt_sample_moves: the legal plane inside the feature planes).
// xa / xb are the logits with NaN replaced by -inf (an ordinary row keeps its bits), so every comparison below is total;
// `deg` marks a degenerate row, whose draw is discarded.  The stored move is -1 or in 0..80 on every path: a drawn mv comes
// from a ballot bit (0..63, 64..80) or is 0, and the replacement's index passes an unsigned bound before it is used.
__global__ __launch_bounds__(64 * SAMPLE_WAVES) void sample_moves_kernel(const float *__restrict__ logits,
                                                                         const uint8_t *__restrict__ mask,
                                                                         size_t mask_stride, int batch,
                                                                         uint32_t k0, uint32_t k1,
                                                                         const uint32_t *__restrict__ counters,
                                                                         int32_t *__restrict__ moves,
                                                                         float *__restrict__ logp) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * SAMPLE_WAVES + (threadIdx.x >> 6);
    if (row >= batch) return;
    const float *x = logits + (size_t)row * P;
    const uint8_t *legal = mask + (size_t)row * mask_stride;
    const bool has1 = lane < P - 64;
    const float ra = x[lane], rb = has1 ? x[64 + lane] : -INFINITY;
    const float xa = is_nan_bits(ra) ? -INFINITY : ra, xb = is_nan_bits(rb) ? -INFINITY : rb;
    float m = fmaxf(xa, xb);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    // degenerate: a NaN or +inf logit, or all 81 at -inf (m is free of NaN: its bits say so)
    const bool deg = __ballot(is_nan_or_pinf(ra) || is_nan_or_pinf(rb)) != 0ull || __float_as_uint(m) == 0xFF800000u;
    const float pa = expf(xa - m), pb = has1 ? expf(xb - m) : 0.f;
    float sa = pa, sb = pb;  // inclusive prefixes of p over points 0..63 and 64..80
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ta = __shfl_up(sa, d), tb = __shfl_up(sb, d);
        if (lane >= d) {
            sa += ta;
            sb += tb;
        }
    }
    sb += __shfl(sa, 63);
    const float S = __shfl(sb, P - 64 - 1);

    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = counters[(size_t)row * 4 + k];
    philox4x32_10(c, k0, k1);
    const float thr = (float)(c[0] >> 8) * 0x1p-24f * S;
    const unsigned long long ga = __ballot(sa > thr), gb = __ballot(has1 && sb > thr);
    int mv;
    if (ga)
        mv = __ffsll(ga) - 1;
    else if (gb)
        mv = 64 + __ffsll(gb) - 1;
    else {  // no prefix above u * S (not expected: u * S < S in fp32): the last point with p > 0
        const unsigned long long za = __ballot(pa > 0.f), zb = __ballot(has1 && pb > 0.f);
        mv = zb ? 64 + 63 - __clzll(zb) : (za ? 63 - __clzll(za) : 0);
    }
    const unsigned long long la = __ballot(legal[lane] != 0), lb = __ballot(has1 && legal[64 + lane] != 0);
    const bool ok = !deg && (mv < 64 ? (la >> mv) & 1ull : (lb >> (mv - 64)) & 1ull);
    if (!ok) {  // an illegal sample, or a degenerate row (no draw counts there)
        if (!(la | lb)) {
            mv = -1;
        } else {  // the legal point of the largest logit (NaN ordered as -inf), lowest index on ties
            float bv = -INFINITY;
            int bi = 1 << 30;
            if ((la >> lane) & 1ull) bv = xa, bi = lane;
            if (((lb >> lane) & 1ull) && (bi == (1 << 30) || xb > bv)) bv = xb, bi = 64 + lane;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const float ov = __shfl_xor(bv, d);
                const int oi = __shfl_xor(bi, d);
                if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
            }
            mv = (unsigned)bi < (unsigned)P ? bi : -1;
        }
    }
    if (lane == 0) {
        moves[row] = mv;
        logp[row] = deg ? __uint_as_float(0x7FC00000u) : (mv >= 0 ? (x[mv] - m) - logf(S) : 0.f);
    }
}

inline hipStream_t S(void *s) { return (hipStream_t)s; }
inline int launched() { return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP; }
inline bool ok_batch(int b) { return b >= 1 && b <= BKT_MAX_BATCH; }
inline bool ok_conv(int cin, int ks) { return cin >= 1 && cin <= 4096 && (ks == 3 || ks == 5); }
inline unsigned blocks(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline int slices_of(int batch) { return (batch + BKT_WGRAD_CHUNK - 1) / BKT_WGRAD_CHUNK; }

}  // namespace

extern "C" {

int bkt_abi_version(void) { return BKT_ABI_VERSION; }

int bkt_conv_pack(const float *w, int cin, int ksize, float *wt, void *stream) {
    if (!w || !wt || !ok_conv(cin, ksize)) return BKT_ERR_ARG;
    const int K = cin * ksize * ksize;
    hipLaunchKernelGGL(pack_kernel, dim3(blocks((size_t)K * BM, 256)), dim3(256), 0, S(stream), w, wt, K);
    return launched();
}

int bkt_conv_pack_dgrad(const float *w, float *wt_dgrad, void *stream) {
    if (!w || !wt_dgrad) return BKT_ERR_ARG;
    hipLaunchKernelGGL(pack_dgrad_kernel, dim3(blocks((size_t)BM * BM * 9, 256)), dim3(256), 0, S(stream), w,
                       wt_dgrad);
    return launched();
}

int bkt_conv_forward(const float *x, const float *wt, const float *bias, float *y, int batch, int cin, int ksize,
                     void *stream) {
    if (!x || !wt || !y || !ok_batch(batch) || !ok_conv(cin, ksize)) return BKT_ERR_ARG;
    const dim3 grid(blocks((size_t)batch * P, BN));
    if (ksize == 5)
        hipLaunchKernelGGL(conv_fwd_kernel<5>, grid, dim3(NT), 0, S(stream), x, wt, bias, y, batch, cin);
    else
        hipLaunchKernelGGL(conv_fwd_kernel<3>, grid, dim3(NT), 0, S(stream), x, wt, bias, y, batch, cin);
    return launched();
}

int bkt_conv_dgrad(const float *dy, const float *wt_dgrad, float *dx, int batch, void *stream) {
    if (!dy || !wt_dgrad || !dx || !ok_batch(batch)) return BKT_ERR_ARG;
    hipLaunchKernelGGL((conv_fwd_kernel<3, true>), dim3(blocks((size_t)batch * P, BN)), dim3(NT), 0, S(stream), dy, wt_dgrad,
                       (const float *)nullptr, dx, batch, BM);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    hipLaunchKernelGGL(dgrad_nonfinite_kernel, dim3(BM), dim3(256), 0, S(stream), dy, wt_dgrad, dx, batch);
    return launched();
}

size_t bkt_bn_workspace(int batch, int channels) {
    if (!ok_batch(batch) || channels < 1 || channels > 4096) return 0;
    return (size_t)slices_of(batch) * channels * 2 * sizeof(double);
}

size_t bkt_conv_wgrad_workspace(int batch, int cin, int ksize) {
    if (!ok_batch(batch) || !ok_conv(cin, ksize)) return 0;
    return bkt_bn_workspace(batch, BM) + (size_t)slices_of(batch) * BM * cin * ksize * ksize * sizeof(float);
}

int bkt_conv_wgrad(const float *x, const float *dy, float *dw, float *db, int batch, int cin, int ksize,
                   void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !dy || !dw || !workspace || !ok_batch(batch) || !ok_conv(cin, ksize)) return BKT_ERR_ARG;
    if (workspace_bytes < bkt_conv_wgrad_workspace(batch, cin, ksize)) return BKT_ERR_ARG;
    const int chunks = slices_of(batch);
    const int NC = cin * ksize * ksize;
    double *bpart = (double *)workspace;
    float *part = (float *)((char *)workspace + bkt_bn_workspace(batch, BM));
    const dim3 grid(blocks(NC, BN), chunks);
    if (ksize == 5)
        hipLaunchKernelGGL(conv_wgrad_kernel<5>, grid, dim3(NT), 0, S(stream), x, dy, part, batch, cin);
    else
        hipLaunchKernelGGL(conv_wgrad_kernel<3>, grid, dim3(NT), 0, S(stream), x, dy, part, batch, cin);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    hipLaunchKernelGGL(chunk_sum_kernel, dim3(blocks((size_t)BM * NC, 256)), dim3(256), 0, S(stream), part, dw,
                       BM * NC, chunks);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    if (db) {
        hipLaunchKernelGGL(chan_partial_kernel<SUM_DY>, dim3(BM, chunks), dim3(RT), 0, S(stream), dy, nullptr, nullptr,
                           nullptr, nullptr, bpart, batch, BM);
        if (launched() != BKT_OK) return BKT_ERR_HIP;
        hipLaunchKernelGGL(chan_sum_finalize_kernel, dim3(1), dim3(256), 0, S(stream), bpart, chunks, db, BM);
        return launched();
    }
    return BKT_OK;
}

int bkt_bn_relu_train(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked, float momentum, float eps, float *y, float *save_mean,
                      float *save_invstd, void *workspace, size_t workspace_bytes, int batch, int channels,
                      void *stream) {
    if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !workspace || !ok_batch(batch) || channels < 1 ||
        channels > 4096 || workspace_bytes < bkt_bn_workspace(batch, channels))
        return BKT_ERR_ARG;
    const int slices = slices_of(batch);
    double *part = (double *)workspace;
    hipLaunchKernelGGL(chan_partial_kernel<SUM_X_XX>, dim3(channels, slices), dim3(RT), 0, S(stream), x, nullptr,
                       nullptr, nullptr, nullptr, part, batch, channels);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(blocks(channels, 256)), dim3(256), 0, S(stream), part, slices,
                       running_mean, running_var, num_batches_tracked, momentum, eps, save_mean, save_invstd, batch,
                       channels);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    const size_t total = (size_t)batch * channels * P;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks(total, 256)), dim3(256), 0, S(stream), x, save_mean, save_invstd,
                       gamma, beta, y, total, channels);
    return launched();
}

int bkt_bn_relu_backward(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                         const float *save_invstd, float *dx, float *dgamma, float *dbeta, void *workspace,
                         size_t workspace_bytes, int batch, int channels, void *stream) {
    if (!dy || !y || !x || !gamma || !save_mean || !save_invstd || !dx || !dgamma || !dbeta || !workspace ||
        !ok_batch(batch) || channels < 1 || channels > 4096 || workspace_bytes < bkt_bn_workspace(batch, channels))
        return BKT_ERR_ARG;
    const int slices = slices_of(batch);
    double *part = (double *)workspace;
    hipLaunchKernelGGL(chan_partial_kernel<SUM_DZ_DZXHAT>, dim3(channels, slices), dim3(RT), 0, S(stream), dy, y, x,
                       save_mean, save_invstd, part, batch, channels);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(blocks(channels, 256)), dim3(256), 0, S(stream), part, slices,
                       dgamma, dbeta, channels);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    const size_t total = (size_t)batch * channels * P;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks(total, 256)), dim3(256), 0, S(stream), dy, y, x, gamma,
                       save_mean, save_invstd, dgamma, dbeta, dx, total, channels, 1.f / (float)(batch * P));
    return launched();
}

int bkt_bn_relu_eval(const float *x, const float *gamma, const float *beta, const float *running_mean,
                     const float *running_var, float eps, float *y, int batch, int channels, void *stream) {
    if (!x || !gamma || !beta || !running_mean || !running_var || !y || !ok_batch(batch) || channels < 1 ||
        channels > 4096)
        return BKT_ERR_ARG;
    const size_t total = (size_t)batch * channels * P;
    hipLaunchKernelGGL(bn_eval_kernel, dim3(blocks(total, 256)), dim3(256), 0, S(stream), x, gamma, beta,
                       running_mean, running_var, eps, y, total, channels);
    return launched();
}

int bkt_bn_relu_eval_backward(const float *dy, const float *y, const float *x, const float *gamma,
                              const float *running_mean, const float *running_var, float eps, float *dx, float *dgamma,
                              float *dbeta, void *workspace, size_t workspace_bytes, int batch, int channels,
                              void *stream) {
    if (!dy || !y || !x || !gamma || !running_mean || !running_var || !dx || !dgamma || !dbeta || !workspace ||
        !ok_batch(batch) || channels < 1 || channels > 4096 || workspace_bytes < bkt_bn_workspace(batch, channels))
        return BKT_ERR_ARG;
    const int slices = slices_of(batch);
    double *part = (double *)workspace;
    hipLaunchKernelGGL(bn_eval_bwd_partial_kernel, dim3(channels, slices), dim3(RT), 0, S(stream), dy, y, x,
                       running_mean, running_var, eps, part, batch, channels);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(blocks(channels, 256)), dim3(256), 0, S(stream), part, slices,
                       dgamma, dbeta, channels);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    const size_t total = (size_t)batch * channels * P;
    hipLaunchKernelGGL(bn_eval_bwd_apply_kernel, dim3(blocks(total, 256)), dim3(256), 0, S(stream), dy, y, gamma,
                       running_var, eps, dx, total, channels);
    return launched();
}

int bkt_sample_moves(const float *logits, const uint8_t *planes, int batch, uint64_t seed, const uint32_t *counters,
                     int32_t *moves, float *logp, void *stream) {
    if (!logits || !planes || !counters || !moves || !logp || batch < 1 || batch > BKT_MAX_SAMPLE_ROWS) return BKT_ERR_ARG;
    return bkt_sample_moves_masked(logits, planes + LEGAL_PLANE * P, (size_t)27 * P, batch, seed, counters, moves, logp,
                                   stream);
}

int bkt_sample_moves_masked(const float *logits, const uint8_t *mask, size_t mask_stride, int batch, uint64_t seed,
                            const uint32_t *counters, int32_t *moves, float *logp, void *stream) {
    if (!logits || !mask || !counters || !moves || !logp || batch < 1 || batch > BKT_MAX_SAMPLE_ROWS) return BKT_ERR_ARG;
    hipLaunchKernelGGL(sample_moves_kernel, dim3(blocks(batch, SAMPLE_WAVES)), dim3(64 * SAMPLE_WAVES), 0, S(stream),
                       logits, mask, mask_stride, batch, (uint32_t)seed, (uint32_t)(seed >> 32), counters, moves, logp);
    return launched();
}

}  // extern "C"

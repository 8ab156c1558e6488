// bk_train_bf16.hip -- the opt-in bf16 mixed-precision convolutions of the 9x9 trunk (include/bokego_train.h, the
// bkt_*_bf16 entry points): forward, input gradient and weight gradient as implicit GEMMs on v_mfma_f32_16x16x32_bf16.
// Self-sufficient: it shares no code with bk_train.hip, whose fp32 kernels stay exactly as they are.
//
// The arithmetic:
//   - Every tensor in memory is fp32 with the fp32 entry points' shapes; only the packed weights are bf16.
//   - Each GEMM operand element is rounded once to bf16, round to nearest even (the __bf16 cast: v_cvt_pk_bf16_f32), on
//     its way into LDS -- the weights in the pack kernel.  Products of two bf16 are exact in fp32; sums are the MFMA's
//     fp32 accumulation, one chain over K per output element.  No Kahan compensation.
//       forward          y  = sum r(w) r(x) + bias      (bias added in fp32, unrounded)
//       input gradient   dx = sum r(w rotated) r(dy)
//       weight gradient  dw = sum r(dy) r(x) per slice of BKT_WGRAD_CHUNK boards, slices added in slice order
//       bias gradient    db = sum of the unrounded dy: double partials per slice, slices added in order
//   - Deterministic: no float atomics, every sum in an order fixed by the shapes alone.
#include <hip/hip_runtime.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int P = 81;                 // points of the board
constexpr int BM = BKT_COUT;          // output channels: one GEMM tile spans all of them
constexpr int BN = 64;                // GEMM columns per workgroup
constexpr int BK = 64;                // reduction depth per LDS stage: two 16x16x32 MFMA k-steps
constexpr int LDP = BK + 8;           // LDS row pitch in bf16 (144 bytes): a lane's 8 k are one aligned 16-byte read, and
                                      // the 16 rows a quarter-wave reads start in 16 different 4-bank groups
constexpr int NT = 256;               // four waves: a 2x2 grid of 64x32 wave tiles
constexpr int RT = 256;               // threads of the per-channel reduction
constexpr int CG = 16;                // forward K order: tap-major, channels padded to a multiple of CG within a tap
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint16_t bf16_bits(float f) {  // round to nearest even; a NaN stays a NaN
    const __bf16 h = (__bf16)f;
    return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) {
    return (uint32_t)bf16_bits(lo) | ((uint32_t)bf16_bits(hi) << 16);
}

__host__ __device__ inline int padded_channels(int cin) { return (cin + CG - 1) / CG * CG; }
__host__ __device__ inline int stages_of(int cin, int ksize) {
    return (padded_channels(cin) * ksize * ksize + BK - 1) / BK;
}

// One BK-deep stage of the 128 x 64 workgroup tile: wave w owns rows (w & 1) * 64 .. +64, columns (w >> 1) * 32 .. +32,
// as 4 x 2 tiles of 16 x 16.  16x16x32 bf16 operands: lane l holds A[l & 15][k = 8 (l >> 4) + j] and
// B[k = 8 (l >> 4) + j][l & 15], j = 0..7.  Both LDS images are [row or column][k], so a fragment is one 16-byte read.
__device__ __forceinline__ void mma_stage(const uint16_t (*As)[LDP], const uint16_t (*Bs)[LDP], f32x4 (&acc)[4][2],
                                          int lane, int wm, int wn) {
    const int c = lane & 15, kq = (lane >> 4) * 8;
#pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
        bf16x8 a[4], b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8 *>(&As[wm + 16 * i + c][ks + kq]);
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const bf16x8 *>(&Bs[wn + 16 * j + c][ks + kq]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

// ---- forward: y[b][m][p] = sum_k wt[m][k] * im2col(x)[k][b*81 + p] (+ bias[m]), k = tap * CP + channel ---------------
// Also the input gradient (wt = the rotated, channel-swapped filters, x = dy, no bias).
// wt is stage-major: [stage][m][BK] bf16, so a stage's 16 KB weight tile is one contiguous, fully coalesced read.
template <int KS>
__global__ __launch_bounds__(NT) void conv_fwd_bf16_kernel(const float *__restrict__ x, const uint16_t *__restrict__ wt,
                                                           const float *__restrict__ bias, float *__restrict__ y,
                                                           int batch, int cin) {
    __shared__ __attribute__((aligned(16))) uint16_t As[BM][LDP];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[BN][LDP];
    constexpr int KK = KS * KS, H = KS / 2;
    const int CP = padded_channels(cin), N = batch * P;
    const int nstages = stages_of(cin, KS);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n0 = blockIdx.x * BN;
    // B (gathered input): this thread owns column bn and the CG consecutive k of group bg: one tap, CG channels.  The
    // lanes of a wave walk consecutive points, so every one of the CG loads is coalesced.  The board point is fixed for
    // the whole K loop; only the tap and the first channel move.
    const int bn = t & (BN - 1), bg = t >> 6;
    const int n = n0 + bn;
    const bool nvalid = n < N;
    const int b = nvalid ? n / P : 0, p = nvalid ? n - (n / P) * P : 0;
    const int py = p / 9, px = p - (p / 9) * 9;
    const float *xb = x + (size_t)b * cin * P;
    const u32x4 *wq = reinterpret_cast<const u32x4 *>(wt);  // 16-byte pieces: 8 per row of a stage

    u32x4 ra[4];
    float rb[CG];
    auto load = [&](int s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = wq[(size_t)s * (BM * BK / 8) + t + NT * i];
        const int kb = s * BK + bg * CG;
        const int tap = kb / CP, c0 = kb - tap * CP;
        const int yy = py + tap / KS - H, xx = px + (tap - (tap / KS) * KS) - H;
        const bool in = nvalid && tap < KK && (unsigned)yy < 9u && (unsigned)xx < 9u;
        const float *src = xb + c0 * P + yy * 9 + xx;
#pragma unroll
        for (int i = 0; i < CG; ++i) rb[i] = (in && c0 + i < cin) ? src[i * P] : 0.f;
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (w & 1) * 64, wn = (w >> 1) * 32;

    load(0);
    for (int s = 0; s < nstages; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = t + NT * i;  // piece q of the stage: row q >> 3, k (q & 7) * 8
            *reinterpret_cast<u32x4 *>(&As[q >> 3][(q & 7) * 8]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < CG; i += 8)
            *reinterpret_cast<u32x4 *>(&Bs[bn][bg * CG + i]) =
                u32x4{bf16_pair(rb[i], rb[i + 1]), bf16_pair(rb[i + 2], rb[i + 3]), bf16_pair(rb[i + 4], rb[i + 5]),
                      bf16_pair(rb[i + 6], rb[i + 7])};
        __syncthreads();
        if (s + 1 < nstages) load(s + 1);  // the next stage's global loads overlap this stage's MFMAs
        mma_stage(As, Bs, acc, lane, wm, wn);
        __syncthreads();
    }

    // C/D of 16x16x32: lane l, register r -> row (l >> 4) * 4 + r, column l & 15
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

// ---- weight gradient: part[chunk][m][n] = sum over the chunk's k = (b, p) of dy[b][m][p] * im2col(x)[n][k] -----------
// The general form (used for k = 5): n = ci * k*k + tap, torch's weight order.  Both operands have k contiguous in memory within a board, so a thread
// loads the two consecutive k of pair kp for its rows and writes them to LDS as one 32-bit word.
template <int KS>
__global__ __launch_bounds__(NT) void conv_wgrad_bf16_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                             float *__restrict__ part, int batch, int cin) {
    __shared__ __attribute__((aligned(16))) uint16_t As[BM][LDP];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[BN][LDP];
    constexpr int KK = KS * KS, H = KS / 2;
    const int NC = cin * KK;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n0 = blockIdx.x * BN, chunk = blockIdx.y;
    const int b_end = min(batch, (chunk + 1) * BKT_WGRAD_CHUNK);
    const int K0 = chunk * BKT_WGRAD_CHUNK * P, K1 = b_end * P;
    // k pair kp = t & 31 (k = 2 kp, 2 kp + 1 of the stage), rows / columns r0 + 8 i
    const int kp = t & 31, r0 = t >> 5;
    int coff[8], cy[8], cx[8];  // the 8 columns of this thread: channel offset and tap displacement; cy = 99 if none
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int nn = n0 + r0 + 8 * i;
        const bool v = nn < NC;
        const int ci = v ? nn / KK : 0, tap = v ? nn - (nn / KK) * KK : 0;
        coff[i] = ci * P;
        cy[i] = v ? tap / KS - H : 99;
        cx[i] = tap - (tap / KS) * KS - H;
    }

    float ra[16][2], rb[8][2];
    auto load = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = k0 + 2 * kp + e;
            const bool kv = k < K1;
            const int b = kv ? k / P : 0, p = kv ? k - (k / P) * P : 0;
            const int py = p / 9, px = p - (p / 9) * 9;
            const float *dyb = dy + (size_t)b * BM * P + p;
            const float *xb = x + (size_t)b * cin * P;
#pragma unroll
            for (int i = 0; i < 16; ++i) ra[i][e] = kv ? dyb[(r0 + 8 * i) * P] : 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int yy = py + cy[i], xx = px + cx[i];
                rb[i][e] = (kv && (unsigned)yy < 9u && (unsigned)xx < 9u) ? xb[coff[i] + yy * 9 + xx] : 0.f;
            }
        }
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (w & 1) * 64, wn = (w >> 1) * 32;

    load(K0);
    for (int k0 = K0; k0 < K1; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            *reinterpret_cast<uint32_t *>(&As[r0 + 8 * i][2 * kp]) = bf16_pair(ra[i][0], ra[i][1]);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<uint32_t *>(&Bs[r0 + 8 * i][2 * kp]) = bf16_pair(rb[i][0], rb[i][1]);
        __syncthreads();
        if (k0 + BK < K1) load(k0 + BK);
        mma_stage(As, Bs, acc, lane, wm, wn);
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

// ---- the 3x3 weight gradient: a 128 x 144 tile of 16 input channels x 9 taps, column tap * 16 + channel -----------------
// A thread's columns are (tap, channel r0) and (tap, channel r0 + 8) for every tap, so the tap of each of its loads is a
// compile-time constant: the board-edge test is shared by the channels of a tap and the tap's displacement is an
// immediate offset of the load.  Wave w owns rows 32 w .. 32 w + 31 and all nine 16-column tiles (one tap each).
constexpr int CT = 16;
constexpr int BN3 = CT * 9;
__global__ __launch_bounds__(NT) void conv_wgrad3_bf16_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                              float *__restrict__ part, int batch, int cin) {
    __shared__ __attribute__((aligned(16))) uint16_t As[BM][LDP];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[BN3][LDP];
    const int NC = cin * 9;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int c0 = blockIdx.x * CT, chunk = blockIdx.y;
    const int b_end = min(batch, (chunk + 1) * BKT_WGRAD_CHUNK);
    const int K0 = chunk * BKT_WGRAD_CHUNK * P, K1 = b_end * P;
    const int kp = t & 31, r0 = t >> 5;  // k pair kp of the stage; rows r0 + 8 i of dy, channels c0 + r0 + 8 h of x
    const bool cv[2] = {c0 + r0 < cin, c0 + r0 + 8 < cin};

    float ra[16][2], rb[18][2];
    auto load = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = k0 + 2 * kp + e;
            const bool kv = k < K1;
            const int b = kv ? k / P : 0, p = kv ? k - (k / P) * P : 0;
            const int py = p / 9, px = p - (p / 9) * 9;
            const float *dyb = dy + ((size_t)b * BM + r0) * P + p;
            const float *xb = x + ((size_t)b * cin + c0 + r0) * P + p;  // read only where cv[h] and the tap is on the board
#pragma unroll
            for (int i = 0; i < 16; ++i) ra[i][e] = kv ? dyb[8 * i * P] : 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ty = tap / 3 - 1, tx = tap % 3 - 1;
                const bool on = kv && (unsigned)(py + ty) < 9u && (unsigned)(px + tx) < 9u;
#pragma unroll
                for (int h = 0; h < 2; ++h) rb[2 * tap + h][e] = (on && cv[h]) ? xb[8 * h * P + ty * 9 + tx] : 0.f;
            }
        }
    };

    f32x4 acc[2][9];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = w * 32, c = lane & 15, kq = (lane >> 4) * 8;

    load(K0);
    for (int k0 = K0; k0 < K1; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            *reinterpret_cast<uint32_t *>(&As[r0 + 8 * i][2 * kp]) = bf16_pair(ra[i][0], ra[i][1]);
#pragma unroll
        for (int j = 0; j < 18; ++j)
            *reinterpret_cast<uint32_t *>(&Bs[(j >> 1) * CT + r0 + 8 * (j & 1)][2 * kp]) = bf16_pair(rb[j][0], rb[j][1]);
        __syncthreads();
        if (k0 + BK < K1) load(k0 + BK);
#pragma unroll
        for (int ks = 0; ks < BK; ks += 32) {
            bf16x8 a[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const bf16x8 *>(&As[wm + 16 * i + c][ks + kq]);
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const bf16x8 bj = *reinterpret_cast<const bf16x8 *>(&Bs[16 * j + c][ks + kq]);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bj, acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    if (c0 + c >= cin) return;
    float *pc = part + (size_t)chunk * BM * NC + (size_t)(c0 + c) * 9;  // column (channel, tap) of torch's weight order
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) pc[(size_t)(wm + 16 * i + (lane >> 4) * 4 + r) * NC + j] = acc[i][j][r];
}

// dw[i] = sum over chunks, in chunk order, of part[chunk][i]
__global__ __launch_bounds__(256) void chunk_sum_bf16_kernel(const float *__restrict__ part, float *__restrict__ dw,
                                                             int n, int chunks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * n + i];
    dw[i] = s;
}

// wt[stage][m][kk], k = stage * BK + kk = tap * CP + c:
//   forward: r(w[m][c][tap]);  dgrad (3x3 128->128): r(w[c][m][8 - tap]), the filters turned by 180 degrees with input
//   and output swapped.  Zero where c >= cin or tap >= k*k (the padding of K).
template <bool DGRAD>
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float *__restrict__ w, uint16_t *__restrict__ wt, int cin,
                                                        int ksize, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int KK = ksize * ksize, CP = padded_channels(cin);
    const int kk = i % BK, m = (i / BK) % BM, s = i / (BK * BM);
    const int k = s * BK + kk, tap = k / CP, c = k - tap * CP;
    float v = 0.f;
    if (tap < KK && c < cin) v = DGRAD ? w[((size_t)c * BM + m) * KK + (KK - 1 - tap)] : w[((size_t)m * cin + c) * KK + tap];
    const uint16_t h = bf16_bits(v);
    if (!DGRAD) {
        wt[i] = h;
        return;
    }
    // the input gradient: a weight that is not finite enters the GEMM as 0 and is kept in the second half of the operand,
    // from where dgrad_nonfinite_bf16_kernel adds it over the taps on the board only
    const bool bad = (h & 0x7F80u) == 0x7F80u;
    wt[i] = bad ? (uint16_t)0 : h;
    wt[total + i] = bad ? h : (uint16_t)0;
}

// bk_train.hip's dgrad_nonfinite_kernel for the packed operand: workgroup m adds w * dy[b][co][p + tap] to dx[b][m][p] for
// each weight of its channel that is not finite, over the taps on the board.  side = the second half of the operand.
__global__ __launch_bounds__(256) void dgrad_nonfinite_bf16_kernel(const float *__restrict__ dy,
                                                                   const uint16_t *__restrict__ side,
                                                                   float *__restrict__ dx, int batch) {
    const int m = blockIdx.x, t = threadIdx.x;
    auto at = [&](int k) { return side[((size_t)(k / BK) * BM + m) * BK + (k % BK)]; };  // k = tap * 128 + co
    int any = 0;
    for (int k = t; k < BM * 9; k += 256) any |= at(k) != 0;
    if (!__syncthreads_or(any)) return;
    for (int i = t; i < batch * P; i += 256) {
        const int b = i / P, p = i - b * P, py = p / 9, px = p - (p / 9) * 9;
        float s = 0.f;
        bool hit = false;
        for (int k = 0; k < BM * 9; ++k) {
            const uint16_t h = at(k);
            if (h == 0) continue;
            const int tap = k / BM, co = k - tap * BM;
            const int yy = py + tap / 3 - 1, xx = px + (tap - (tap / 3) * 3) - 1;
            if ((unsigned)yy < 9u && (unsigned)xx < 9u) {
                s += __uint_as_float((uint32_t)h << 16) * dy[((size_t)b * BM + co) * P + yy * 9 + xx];
                hit = true;
            }
        }
        if (hit) dx[((size_t)b * BM + m) * P + p] += s;
    }
}

// ---- db: per-channel sums of the unrounded dy, as bk_train.hip's SUM_DY reduction: workgroup (c, s) sums slice s
// (boards 16 s .. 16 s + 15) of channel c in double -- a thread's strided serial sum, then an LDS tree -- and a finalize
// kernel adds the slices of a channel in slice order.
__global__ __launch_bounds__(RT) void dy_partial_kernel(const float *__restrict__ dy, double *__restrict__ part,
                                                        int batch) {
    __shared__ double sh[RT];
    const int c = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    const int b0 = s * BKT_WGRAD_CHUNK, nb = min(batch - b0, BKT_WGRAD_CHUNK);
    double s0 = 0.0;
    for (int i = t; i < nb * P; i += RT) {
        const int b = b0 + i / P;
        s0 += dy[((size_t)b * BM + c) * P + (i - (i / P) * P)];
    }
    sh[t] = s0;
    __syncthreads();
#pragma unroll
    for (int d = RT / 2; d > 0; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    if (t == 0) part[(size_t)s * BM + c] = sh[0];
}

__global__ __launch_bounds__(BM) void dy_finalize_kernel(const double *__restrict__ part, int slices,
                                                         float *__restrict__ db) {
    const int c = threadIdx.x;
    double s0 = 0.0;
    for (int s = 0; s < slices; ++s) s0 += part[(size_t)s * BM + c];
    db[c] = (float)s0;
}

inline hipStream_t S(void *s) { return (hipStream_t)s; }
inline int launched() { return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP; }
inline bool ok_batch(int b) { return b >= 1 && b <= BKT_MAX_BATCH; }
inline bool ok_conv(int cin, int ks) { return cin >= 1 && cin <= 4096 && (ks == 3 || ks == 5); }
inline unsigned blocks(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline int slices_of(int batch) { return (batch + BKT_WGRAD_CHUNK - 1) / BKT_WGRAD_CHUNK; }
inline size_t db_bytes(int batch) { return (size_t)slices_of(batch) * BM * 2 * sizeof(double); }  // bkt_bn_workspace's

}  // namespace

extern "C" {

size_t bkt_conv_packed_elems_bf16(int cin, int ksize) {
    if (!ok_conv(cin, ksize)) return 0;
    const size_t n = (size_t)stages_of(cin, ksize) * BM * BK;
    return cin == BM && ksize == 3 ? 2 * n : n;  // room for the input gradient's weights that are not finite (pack_bf16_kernel)
}

int bkt_conv_pack_bf16(const float *w, int cin, int ksize, uint16_t *wt, void *stream) {
    if (!w || !wt || !ok_conv(cin, ksize)) return BKT_ERR_ARG;
    const int total = stages_of(cin, ksize) * BM * BK;
    hipLaunchKernelGGL(pack_bf16_kernel<false>, dim3(blocks(total, 256)), dim3(256), 0, S(stream), w, wt, cin, ksize,
                       total);
    return launched();
}

int bkt_conv_pack_dgrad_bf16(const float *w, uint16_t *wt_dgrad, void *stream) {
    if (!w || !wt_dgrad) return BKT_ERR_ARG;
    const int total = stages_of(BM, 3) * BM * BK;
    hipLaunchKernelGGL(pack_bf16_kernel<true>, dim3(blocks(total, 256)), dim3(256), 0, S(stream), w, wt_dgrad, BM, 3,
                       total);
    return launched();
}

int bkt_conv_forward_bf16(const float *x, const uint16_t *wt, const float *bias, float *y, int batch, int cin, int ksize,
                          void *stream) {
    if (!x || !wt || !y || !ok_batch(batch) || !ok_conv(cin, ksize)) return BKT_ERR_ARG;
    const dim3 grid(blocks((size_t)batch * P, BN));
    if (ksize == 5)
        hipLaunchKernelGGL(conv_fwd_bf16_kernel<5>, grid, dim3(NT), 0, S(stream), x, wt, bias, y, batch, cin);
    else
        hipLaunchKernelGGL(conv_fwd_bf16_kernel<3>, grid, dim3(NT), 0, S(stream), x, wt, bias, y, batch, cin);
    return launched();
}

int bkt_conv_dgrad_bf16(const float *dy, const uint16_t *wt_dgrad, float *dx, int batch, void *stream) {
    const int rc = bkt_conv_forward_bf16(dy, wt_dgrad, nullptr, dx, batch, BM, 3, stream);
    if (rc != BKT_OK) return rc;
    hipLaunchKernelGGL(dgrad_nonfinite_bf16_kernel, dim3(BM), dim3(256), 0, S(stream), dy,
                       wt_dgrad + (size_t)stages_of(BM, 3) * BM * BK, dx, batch);
    return launched();
}

size_t bkt_conv_wgrad_workspace_bf16(int batch, int cin, int ksize) {
    if (!ok_batch(batch) || !ok_conv(cin, ksize)) return 0;
    return db_bytes(batch) + (size_t)slices_of(batch) * BM * cin * ksize * ksize * sizeof(float);
}

int bkt_conv_wgrad_bf16(const float *x, const float *dy, float *dw, float *db, int batch, int cin, int ksize,
                        void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !dy || !dw || !workspace || !ok_batch(batch) || !ok_conv(cin, ksize)) return BKT_ERR_ARG;
    if (workspace_bytes < bkt_conv_wgrad_workspace_bf16(batch, cin, ksize)) return BKT_ERR_ARG;
    const int chunks = slices_of(batch);
    const int NC = cin * ksize * ksize;
    double *bpart = (double *)workspace;
    float *part = (float *)((char *)workspace + db_bytes(batch));
    if (ksize == 5)
        hipLaunchKernelGGL(conv_wgrad_bf16_kernel<5>, dim3(blocks(NC, BN), chunks), dim3(NT), 0, S(stream), x, dy, part,
                           batch, cin);
    else
        hipLaunchKernelGGL(conv_wgrad3_bf16_kernel, dim3(blocks(cin, CT), chunks), dim3(NT), 0, S(stream), x, dy, part,
                           batch, cin);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    hipLaunchKernelGGL(chunk_sum_bf16_kernel, dim3(blocks((size_t)BM * NC, 256)), dim3(256), 0, S(stream), part, dw,
                       BM * NC, chunks);
    if (launched() != BKT_OK) return BKT_ERR_HIP;
    if (db) {
        hipLaunchKernelGGL(dy_partial_kernel, dim3(BM, chunks), dim3(RT), 0, S(stream), dy, bpart, batch);
        if (launched() != BKT_OK) return BKT_ERR_HIP;
        hipLaunchKernelGGL(dy_finalize_kernel, dim3(1), dim3(BM), 0, S(stream), bpart, chunks, db);
        return launched();
    }
    return BKT_OK;
}

}  // extern "C"

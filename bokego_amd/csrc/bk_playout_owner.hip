// bk_playout_owner.hip -- what the final boards of whole playouts say beyond who won: bkt_owner_counts
// (include/bokego_train.h has the definition) scores the n final records of every start record as bkt_area_score does and
// reduces them, in the same launch, to integer ownership, agreement and score-margin counts (bokego_amd/rollout.py
// playout_ownership).  No owner array reaches memory.  A translation unit of its own in libbktrain.so, beside
// bk_playout_amaf.hip and bk_playout_rave.hip: bk_playout.hip and the text-include chain above it stay exactly as the
// resource tests pin them, so the bitboard helpers below -- BB, dilate, meets, the ballot publish and position_set -- are
// that file's and bk_encode_dev.h's, repeated here on purpose.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bokego_go.h"
#include "../../include/bokego_train.h"

namespace {

constexpr int NN = 81;                    // points of the board
constexpr int PPW = 3;                    // boards of one round: 3 * 81 = 243 of the 256 threads have a point
constexpr int POS_BYTES = 192;            // sizeof(bk_pos)
constexpr int BINS = 2 * NN + 1;          // margins -81 .. 81
constexpr unsigned M27 = 0x7FFFFFFu;      // one word = 3 board rows
constexpr unsigned NC0 = 0x1FEu | (0x1FEu << 9) | (0x1FEu << 18);  // points whose column is not 0
constexpr unsigned NC8 = 0x0FFu | (0x0FFu << 9) | (0x0FFu << 18);  // points whose column is not 8

struct BB {  // 81-point set: word k = rows 3k..3k+2, bit = 9*(row%3) + col
    unsigned w[3];
};
__device__ __forceinline__ BB operator|(BB a, BB b) { return {{a.w[0] | b.w[0], a.w[1] | b.w[1], a.w[2] | b.w[2]}}; }
__device__ __forceinline__ BB operator&(BB a, BB b) { return {{a.w[0] & b.w[0], a.w[1] & b.w[1], a.w[2] & b.w[2]}}; }
__device__ __forceinline__ BB operator~(BB a) { return {{~a.w[0] & M27, ~a.w[1] & M27, ~a.w[2] & M27}}; }
__device__ __forceinline__ bool operator!=(BB a, BB b) { return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2])) != 0; }
__device__ __forceinline__ int popc(BB a) { return __popc(a.w[0]) + __popc(a.w[1]) + __popc(a.w[2]); }
__device__ __forceinline__ bool meets(BB a, BB b) { return ((a.w[0] & b.w[0]) | (a.w[1] & b.w[1]) | (a.w[2] & b.w[2])) != 0; }
// all points adjacent to a point of x
__device__ __forceinline__ BB dilate(BB x) {
    BB d;
    d.w[0] = ((x.w[0] << 9) & M27) | (x.w[0] >> 9) | ((x.w[1] << 18) & M27) | ((x.w[0] << 1) & NC0) | ((x.w[0] >> 1) & NC8);
    d.w[1] = ((x.w[1] << 9) & M27) | (x.w[0] >> 18) | (x.w[1] >> 9) | ((x.w[2] << 18) & M27) | ((x.w[1] << 1) & NC0) | ((x.w[1] >> 1) & NC8);
    d.w[2] = ((x.w[2] << 9) & M27) | (x.w[1] >> 18) | (x.w[2] >> 9) | ((x.w[2] << 1) & NC0) | ((x.w[2] >> 1) & NC8);
    return d;
}
__device__ __forceinline__ BB single(int k, unsigned bit) {  // no dynamic register indexing
    return {{k == 0 ? bit : 0u, k == 1 ? bit : 0u, k == 2 ? bit : 0u}};
}
__device__ __forceinline__ void publish_ballots(unsigned (&bal)[2][8], int tid, bool a, bool b) {
    const unsigned long long ba = __ballot(a), bb = __ballot(b);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        bal[0][2 * w] = (unsigned)ba; bal[0][2 * w + 1] = (unsigned)(ba >> 32);
        bal[1][2 * w] = (unsigned)bb; bal[1][2 * w + 1] = (unsigned)(bb >> 32);
    }
}
__device__ __forceinline__ BB position_set(const unsigned (&bal)[8], int p) {   // the 81 bits of seat p < PPW
    BB s;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
        const int off = NN * p + 27 * kk, i = off >> 5, sh = off & 31;           // off + 27 <= 243: i + 1 <= 7
        s.w[kk] = (unsigned)((((unsigned long long)bal[i + 1] << 32) | bal[i]) >> sh) & M27;
    }
    return s;
}

struct OwnerLds {                         // 5012 bytes
    unsigned stones[2][8], area[2][8];    // the ballots of the 4 waves = 256 bits each: black | white stones, black | white area
    int32_t part[PPW][3][NN];             // [seat][black | white | agree][point]
    int32_t bins[PPW][BINS];              // [seat][margin + 81]
    int32_t wins[PPW];                    // [seat] rows black won
};

// One workgroup per record r; a round takes PPW of the record's boards in area_score_kernel's seating: thread (p, q) is
// point q of board j0 + p.  Per round:
//   ballots of the stones, ONE barrier, the flood of the empty regions by dilate (wave-uniform exit) and the meets test:
//   own, exactly area_score_kernel's;  ballots of the two areas, ONE barrier;  every thread of a seat takes B and W from the
//   popcounts of its board's area sets, so it knows bw without a third barrier, and adds own and agreement of its point to
//   three registers;  the q == 0 thread of the seat bumps the seat's own histogram bin and win counter in LDS -- one array
//   per seat, one writer each, no atomics.
// The board byte of the next round is loaded before this round's flood.  A seat beyond the record's last board (a tail
// round: playouts need not be a multiple of PPW) loads nothing and counts nothing.  The buffers need no third barrier:
// `stones` is last read before the round's second barrier and next written after it, `area` is last read before the next
// round's first barrier and next written after it.  At the end the seats' partial results meet in LDS; thread t < 243 adds
// the three of (array, point) = (t / 81, t % 81), thread t < 163 the three of margin bin t, thread 255 the wins: plain
// vector stores.  Loop bounds and barriers depend on `playouts` alone.  Integers only but for the one comparison that is
// area_score_kernel's expression.  What is read: the 81 board bytes of the rows r * playouts .. (r + 1) * playouts - 1.
__global__ void __launch_bounds__(256) owner_counts_kernel(const unsigned char* __restrict__ pos, int playouts, float komi,
                                                           int32_t* __restrict__ black, int32_t* __restrict__ white,
                                                           int32_t* __restrict__ agree, int32_t* __restrict__ hist,
                                                           int32_t* __restrict__ black_wins) {
    __shared__ OwnerLds S;
    unsigned (&stones)[2][8] = S.stones, (&area)[2][8] = S.area;
    int32_t (&part)[PPW][3][NN] = S.part, (&bins)[PPW][BINS] = S.bins, (&wins)[PPW] = S.wins;
    const int tid = threadIdx.x;
    const int p = tid / NN, q = tid - NN * p;
    const bool seated = p < PPW;                                        // threads 243..255 have no point
    const int pp = seated ? p : 0;
    const int k = q / 27;
    const BB me = single(k, 1u << (q - 27 * k));
    const unsigned char* src = pos + ((size_t)blockIdx.x * playouts + pp) * POS_BYTES + q;   // this thread's byte of round 0

    for (int i = tid; i < PPW * BINS; i += 256) (&bins[0][0])[i] = 0;   // (read after the first round's barriers)
    if (tid < PPW) wins[tid] = 0;
    int nb = 0, nw = 0, na = 0;
    int next = seated && p < playouts ? src[0] : 0;
    for (int j0 = 0; j0 < playouts; j0 += PPW) {
        const bool live = seated && j0 + p < playouts;
        const int me_board = next;
        src += (size_t)PPW * POS_BYTES;
        next = seated && j0 + PPW + p < playouts ? src[0] : 0;

        publish_ballots(stones, tid, me_board == BK_BLACK, me_board == BK_WHITE);
        __syncthreads();
        const BB bl = position_set(stones[0], pp), wh = position_set(stones[1], pp);
        const BB empty = ~(bl | wh);
        BB x = me;
        bool changed = live && me_board == BK_EMPTY;
        BB d = dilate(x);
        for (;;) {                         // wave-uniform exit
            const BB nx = (x | d) & empty;
            changed = changed && (nx != x);
            if (!__any(changed)) break;
            if (changed) x = nx;
            d = dilate(x);
        }
        int own = me_board == BK_BLACK ? 1 : me_board == BK_WHITE ? -1 : 0;
        if (live && me_board == BK_EMPTY) own = (int)meets(d, bl) - (int)meets(d, wh);

        publish_ballots(area, tid, live && own > 0, live && own < 0);
        __syncthreads();
        if (!live) continue;               // (the loop and its barriers go on: j0 is uniform)
        const int B = popc(position_set(area[0], p)), W = popc(position_set(area[1], p));
        const bool bw = ((float)B - ((float)W + komi)) > 0.0f;
        nb += own > 0, nw += own < 0;
        na += (own > 0 && bw) || (own < 0 && !bw);
        if (q == 0) {
            bins[p][B - W + NN] += 1;
            wins[p] += bw;
        }
    }
    if (seated) part[p][0][q] = nb, part[p][1][q] = nw, part[p][2][q] = na;
    __syncthreads();
    const size_t r = blockIdx.x;
    if (tid < 3 * NN) {
        const int32_t* p0 = &part[0][0][0] + tid;                       // (array, point) = (tid / 81, tid % 81)
        int32_t* out = p == 0 ? black : p == 1 ? white : agree;
        out[r * NN + q] = p0[0] + p0[3 * NN] + p0[6 * NN];
    }
    if (tid < BINS) hist[r * BINS + tid] = bins[0][tid] + bins[1][tid] + bins[2][tid];
    if (tid == 255) black_wins[r] = wins[0] + wins[1] + wins[2];
}

}  // namespace

extern "C" int bkt_owner_counts(const void* pos, int records, int playouts, float komi, int32_t* black, int32_t* white,
                                int32_t* agree, int32_t* hist, int32_t* black_wins, void* stream) {
    if (!pos || !black || !white || !agree || !hist || !black_wins || records < 1 || playouts < 1 ||
        (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || !(komi - komi == 0.0f))                  // komi finite
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(owner_counts_kernel, dim3(records), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), playouts, komi, black, white, agree, hist, black_wins);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

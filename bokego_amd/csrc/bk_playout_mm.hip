// bk_playout_mm.hip -- one minorization-maximization (MM) pass over packed positions, for the joint fit of the pattern
// and the tactics table (bokego_amd/mmfit.py): bkt_mm_sums (include/bokego_train.h has the definition).  A
// translation unit of its own in libbktrain.so, as bk_playout_amaf.hip is: it reads packed codes and two strength tables
// and nothing of the playout kernels, whose text-include chain and pinned resources stay as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int NN = 81;                        // points of the board
constexpr int SEATS = 3;                      // rows of a round: thread t < 243 is point t % 81 of row slot t / 81 (the encoder's seating)
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int HOT = 512;                      // stone-free pattern indices, kept in LDS (below)
constexpr int MAX_BLOCKS = 1024;
typedef unsigned long long u64;

__device__ inline u64 shfl_xor_u64(u64 v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return (u64)hi << 32 | lo;
}

// A pattern index whose eight neighbours are all empty or off the board (2-bit states 0 and 3 only): the indices of an
// empty region, 2^8 x near.  From the empty board every point of every row has one of them, and index 0 is the hottest
// address of a whole data set, so what a workgroup adds to them is summed in LDS and leaves once, at the end.
__device__ inline bool stone_free(uint32_t i) { return (((i ^ (i >> 1)) & 0x5555u)) == 0; }
__device__ inline uint32_t hot_slot(uint32_t i) {          // the even bits of the low 16, packed, | near << 8
    uint32_t x = i & 0x5555u;
    x = (x | x >> 1) & 0x3333u, x = (x | x >> 2) & 0x0F0Fu, x = (x | x >> 4) & 0x00FFu;
    return x | (i >> 16 & 1u) << 8;
}
__device__ inline uint32_t hot_index(uint32_t slot) {      // hot_slot's inverse
    uint32_t x = slot & 0xFFu;
    x = (x | x << 4) & 0x0F0Fu, x = (x | x << 2) & 0x3333u, x = (x | x << 1) & 0x5555u;
    return x * 3u | (slot >> 8 & 1u) << 16;
}

// A round seats SEATS rows; a workgroup walks rounds blockIdx.x, blockIdx.x + gridDim.x, ... (bounds and barriers depend on
// blockIdx and rows alone: workgroup-uniform).  Per round:
//   A  every thread reads its point's word and forms s; a row's 81 threads lie in two waves, so each wave reduces s over
//      the lanes of its first row slot and of the next one (butterfly), and lane 0 leaves the two partial sums in LDS; the
//      thread of the played point leaves s_m (0: the row adds nothing);
//   B  after a barrier every thread has E and s_m of its row: rank by ballot, and the two quotients of the point.  Points
//      of a wave with the same word in the same row have the same quotients, so the wave adds them together: a leader per
//      distinct (word, row) adds count x quotient -- to den_t in LDS, to den_p in LDS (stone-free indices) or by ONE 64-bit
//      integer atomicAdd on global memory.  Integer sums: the result does not depend on the order;
//   C  after a second barrier the first thread of each row writes total, chosen and rank.
// Every index is masked before use (17 bits into gp and den_p, 6 bits into gt and den_t) and every row is compared
// with `rows`, so no input can make the kernel read or write outside its buffers.  E reaches a division only for a row
// with a playable played point, where E >= s_m >= 1.
__global__ void __launch_bounds__(THREADS) mm_sums_kernel(const uint32_t* __restrict__ codes, const int32_t* __restrict__ moves,
                                                          int rows, const uint32_t* __restrict__ gp, const uint32_t* __restrict__ gt,
                                                          u64* __restrict__ den_p, u64* __restrict__ den_t, u64* __restrict__ total,
                                                          u64* __restrict__ chosen, int32_t* __restrict__ rank) {
    __shared__ u64 hot[HOT];
    __shared__ u64 dt[BKT_TACTIC_ENTRIES];
    __shared__ uint32_t gts[BKT_TACTIC_ENTRIES];
    __shared__ u64 part_e[WAVES][2];
    __shared__ u64 s_played[SEATS];
    __shared__ int part_r[WAVES][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q = tid / NN, j = tid - q * NN;                          // q == SEATS: the 13 idle threads
    const int q_lo = (wave * 64) / NN;                                 // the row slot of the wave's first lane; the others: q_lo or q_lo + 1
    const bool upper = q != q_lo;
    for (int i = tid; i < HOT; i += THREADS) hot[i] = 0;
    if (tid < BKT_TACTIC_ENTRIES) dt[tid] = 0, gts[tid] = gt[tid];
    __syncthreads();
    for (int base = blockIdx.x * SEATS; base < rows; base += gridDim.x * SEATS) {
        const int r = base + q;
        const bool live = q < SEATS && r < rows;
        const uint32_t word = live ? codes[(size_t)r * NN + j] : 0u;
        const int m = live ? moves[r] : -1;
        const bool playable = word >> 31;
        const uint32_t idx = word & (BKT_PATTERN_ENTRIES - 1), code = word >> 17 & (BKT_TACTIC_ENTRIES - 1);
        const u64 g_p = playable ? gp[idx] : 0u, g_t = gts[code];
        u64 s = 0;
        if (playable) s = (g_p * g_t) >> 16, s = s < 1 ? 1 : s;
        const bool on_board = m >= 0 && m < NN;
        if (live && j == (on_board ? m : 0)) s_played[q] = on_board ? s : 0;
        u64 e0 = upper ? 0 : s, e1 = upper ? s : 0;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) e0 += shfl_xor_u64(e0, k), e1 += shfl_xor_u64(e1, k);
        if (lane == 0) part_e[wave][0] = e0, part_e[wave][1] = e1;
        __syncthreads();
        u64 E = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if ((w * 64) / NN + k == q) E += part_e[w][k];
        const u64 s_m = live ? s_played[q] : 0;
        const bool counts = s_m > 0 && playable;                       // a point of a row that adds to the sums
        const u64 beats = __ballot(counts && (s > s_m || (s == s_m && j < m)));
        const u64 uppers = __ballot(upper);
        if (lane == 0) part_r[wave][0] = __popcll(beats & ~uppers), part_r[wave][1] = __popcll(beats & uppers);
        u64 add_p = 0, add_t = 0;
        if (counts) add_p = (g_t << 32) / E, add_t = (g_p << 32) / E;
        const int key = (int)((word & 0x7FFFFFu) | (uint32_t)q << 23);
        bool waiting = counts;
        for (u64 rest = __ballot(waiting); rest; rest = __ballot(waiting)) {
            const int leader = __ffsll(rest) - 1;
            const bool mine = waiting && key == __shfl(key, leader);
            const u64 n = __popcll(__ballot(mine));
            if (lane == leader) {
                if (stone_free(idx)) atomicAdd(&hot[hot_slot(idx)], n * add_p);
                else atomicAdd(&den_p[idx], n * add_p);
                atomicAdd(&dt[code], n * add_t);
            }
            waiting = waiting && !mine;
        }
        __syncthreads();
        if (live && j == 0) {
            int above = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w)
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if ((w * 64) / NN + k == q) above += part_r[w][k];
            total[r] = E, chosen[r] = s_m, rank[r] = s_m > 0 ? above : -1;
        }
    }
    __syncthreads();
    for (int i = tid; i < HOT; i += THREADS)
        if (hot[i]) atomicAdd(&den_p[hot_index(i)], hot[i]);
    if (tid < BKT_TACTIC_ENTRIES && dt[tid]) atomicAdd(&den_t[tid], dt[tid]);
}

}  // namespace

extern "C" int bkt_mm_sums(const uint32_t* codes, const int32_t* moves, int rows, const uint32_t* gp, const uint32_t* gt,
                           uint64_t* den_p, uint64_t* den_t, uint64_t* total, uint64_t* chosen, int32_t* rank, void* stream) {
    if (!codes || !moves || !gp || !gt || !den_p || !den_t || !total || !chosen || !rank || rows < 1 || rows > BKT_MM_MAX_ROWS)
        return BKT_ERR_ARG;
    const int rounds = (rows + SEATS - 1) / SEATS;
    hipLaunchKernelGGL(mm_sums_kernel, dim3(rounds < MAX_BLOCKS ? rounds : MAX_BLOCKS), dim3(THREADS), 0, (hipStream_t)stream,
                       codes, moves, rows, gp, gt, (u64*)den_p, (u64*)den_t, (u64*)total, (u64*)chosen, rank);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

// bk_playout_rave.hip -- the two-sided all-moves-as-first (AMAF) counts of whole playouts, the records the tree's RAVE tables
// are made of (bk_tree.cpp, bk_pool_deliver_rave): bkt_amaf_counts_sides (include/bokego_train.h has the
// definition).  A translation unit of its own in libbktrain.so, beside bk_playout_amaf.hip, whose kernel stays exactly as
// the resource tests pin it: the staging loop below is that kernel's, repeated here on purpose.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int NN = 81;                       // points of the board
constexpr int WAVES = 4;                     // waves of a workgroup: the playouts of one barrier round, one per wave
constexpr int ROW = BKT_MAX_PLAYOUT_PLIES;   // int16 entries of a staged row (a multiple of 4: the scan reads 4 at a time)

// amaf_counts_kernel (bk_playout_amaf.hip) with both halves of every history kept.  One workgroup per record r; a round
// takes WAVES playouts of the record:
//   stage  the whole workgroup copies their adjacent rows of `moves` into LDS, thread t the entries t, t + 256, ... of each
//          row (coalesced 2-byte loads), padded with BKT_MOVE_NONE to a multiple of 4 entries;
//   scan   after ONE barrier wave w owns playout j0 + w: lane l looks for the first ply of the points l and l + 64 (l < 17)
//          by broadcast 8-byte LDS reads (every lane reads the same address), so the walk and its end at the first entry
//          <= BKT_MOVE_NONE or at max_plies are uniform in the wave.  The parity of that first ply is the side the row
//          counts for: ply k + e with k a multiple of 4 has the parity of e.
// Two LDS buffers alternate, so a round costs one barrier.  The counts -- eight per lane: played and won_at of two points
// for two sides -- stay in registers until the end; there the waves' partial counts meet in LDS and thread t < 2 * 81 adds
// the four of (side, point) = (t / 81, t % 81) and writes played[r, side, s] and won_at[r, side, s] with plain stores.
// Integers only, no atomics; loop bounds and barriers depend on `playouts` and `max_plies` alone (workgroup-uniform).
// What is read: moves[row, k] for row < records * playouts and k < max_plies, won[row] for the same rows.  An entry is only
// compared, never used as an index: one above 80 matches no point, one below BKT_MOVE_NONE ends the row as that does.
__global__ void __launch_bounds__(64 * WAVES) amaf_counts_sides_kernel(const int16_t* __restrict__ moves, int max_plies,
                                                                       const uint8_t* __restrict__ won, int playouts,
                                                                       int32_t* __restrict__ played,
                                                                       int32_t* __restrict__ won_at) {
    __shared__ __attribute__((aligned(8))) int16_t rows[2][WAVES][ROW];
    __shared__ int32_t part[WAVES][2][2][NN];                          // [wave][played | won_at][side][point]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)blockIdx.x * playouts;                 // the record's first row
    const int padded = (max_plies + 3) & ~3;                           // <= ROW
    const int s0 = lane, s1 = lane < NN - 64 ? lane + 64 : -100;       // -100: no entry that is compared equals it
    int n00 = 0, n01 = 0, n10 = 0, n11 = 0;                            // played[side][s0 | s1] of this wave's playouts
    int w00 = 0, w01 = 0, w10 = 0, w11 = 0;                            // won_at likewise
    int buf = 0;
    for (int j0 = 0; j0 < playouts; j0 += WAVES, buf ^= 1) {
        const int here = min(WAVES, playouts - j0);
        const int16_t* src = moves + (row0 + j0) * max_plies;
        for (int i = tid; i < padded; i += 64 * WAVES) {                // the round's loads first: WAVES in flight per thread
            int16_t e[WAVES];
#pragma unroll
            for (int w = 0; w < WAVES; ++w)
                e[w] = w < here && i < max_plies ? src[(size_t)w * max_plies + i] : (int16_t)BKT_MOVE_NONE;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) rows[buf][w][i] = e[w];
        }
        __syncthreads();
        if (wave >= here) continue;                                    // (the loop and its barrier go on: j0 is uniform)
        const bool win = won[row0 + j0 + wave] != 0;
        const int16_t* row = rows[buf][wave];
        bool seen0 = false, seen1 = false, odd0 = false, odd1 = false;
        bool live = true;
        for (int k = 0; k < padded && live; k += 4) {
            const uint2 v = *reinterpret_cast<const uint2*>(row + k);
            const int m[4] = {(int16_t)(v.x & 0xFFFFu), (int16_t)(v.x >> 16), (int16_t)(v.y & 0xFFFFu), (int16_t)(v.y >> 16)};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                live = live && m[e] > BKT_MOVE_NONE;
                const bool odd = (e & 1) != 0;                         // ply k + e is odd: k is a multiple of 4
                if (live && !seen0 && m[e] == s0) seen0 = true, odd0 = odd;
                if (live && !seen1 && m[e] == s1) seen1 = true, odd1 = odd;
            }
        }
        // side 0 is the side to move at the record and wins the rows with won != 0; side 1 wins the others
        const bool a0 = seen0 && !odd0, b0 = seen0 && odd0, a1 = seen1 && !odd1, b1 = seen1 && odd1;
        n00 += a0, w00 += a0 && win, n10 += b0, w10 += b0 && !win;
        n01 += a1, w01 += a1 && win, n11 += b1, w11 += b1 && !win;
    }
    part[wave][0][0][s0] = n00, part[wave][0][1][s0] = n10, part[wave][1][0][s0] = w00, part[wave][1][1][s0] = w10;
    if (s1 >= 0) part[wave][0][0][s1] = n01, part[wave][0][1][s1] = n11, part[wave][1][0][s1] = w01, part[wave][1][1][s1] = w11;
    __syncthreads();
    if (tid < 2 * NN) {                                                // (side, point) = (tid / 81, tid % 81): [r, 2, 81] in order
        int n = 0, w = 0;
        const int32_t* p0 = &part[0][0][0][0] + tid;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) n += p0[v * 4 * NN], w += p0[v * 4 * NN + 2 * NN];
        played[(size_t)blockIdx.x * 2 * NN + tid] = n;
        won_at[(size_t)blockIdx.x * 2 * NN + tid] = w;
    }
}

}  // namespace

extern "C" int bkt_amaf_counts_sides(const int16_t* moves, int max_plies, const uint8_t* won, int records, int playouts,
                                     int32_t* played, int32_t* won_at, void* stream) {
    if (!moves || !won || !played || !won_at || records < 1 || playouts < 1 ||
        (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 || max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(amaf_counts_sides_kernel, dim3(records), dim3(64 * WAVES), 0, (hipStream_t)stream, moves, max_plies,
                       won, playouts, played, won_at);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

// bk_playout_amaf.hip -- the all-moves-as-first (AMAF) counts of whole playouts, for the search prior of
// bokego_amd/rollout.py (playout_amaf, amaf_prior): bkt_amaf_counts (include/bokego_train.h).  A translation unit
// of its own in libbktrain.so: it reads the move history the bkt_*_playouts calls write and nothing else of theirs, and
// the text-include chain of bk_playout*.hip, whose kernels the resource tests pin, stays as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int NN = 81;                       // points of the board
constexpr int WAVES = 4;                     // waves of a workgroup: the playouts of one barrier round, one per wave
constexpr int ROW = BKT_MAX_PLAYOUT_PLIES;   // int16 entries of a staged row (a multiple of 4: the scan reads 4 at a time)

// One workgroup per record r; its 81 x 2 counters never leave the workgroup.  A round takes WAVES playouts of the record:
//   stage  their rows of `moves` are adjacent in memory; the whole workgroup copies them into LDS, thread t the entries t,
//          t + 256, ... of each row (coalesced 2-byte loads), padded with BKT_MOVE_NONE to a multiple of 4 entries;
//   scan   after ONE barrier wave w owns playout j0 + w: lane l looks for the first ply of the points l and l + 64 (l < 17).
//          Every lane of the wave reads the same LDS address -- a broadcast, 4 entries per 8-byte read -- so the walk, and
//          its end at the first entry <= BKT_MOVE_NONE or at max_plies, is uniform in the wave: no divergence, and the
//          search for a point's first ply is two compares and two selects per entry.
// Two LDS buffers alternate, so a round costs one barrier: the buffer a round stages into was scanned two rounds ago, and
// every wave has passed the barrier in between.  The counts stay in registers until the end; there the waves' partial
// counts meet in LDS and thread s < 81 adds the four of point s and writes played[r, s] and won_at[r, s] with plain stores.
// Integers only, no atomics; loop bounds and barriers depend on `playouts` and `max_plies` alone (workgroup-uniform).
// What is read: moves[row, k] for row < records * playouts and k < max_plies, won[row] for the same rows.  An entry is only
// compared, never used as an index: one above 80 matches no point, one below BKT_MOVE_NONE ends the row as that does.
__global__ void __launch_bounds__(64 * WAVES) amaf_counts_kernel(const int16_t* __restrict__ moves, int max_plies,
                                                                 const uint8_t* __restrict__ won, int playouts,
                                                                 int32_t* __restrict__ played, int32_t* __restrict__ won_at) {
    __shared__ __attribute__((aligned(8))) int16_t rows[2][WAVES][ROW];
    __shared__ int32_t part[WAVES][2][NN];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)blockIdx.x * playouts;                 // the record's first row
    const int padded = (max_plies + 3) & ~3;                           // <= ROW
    const int s0 = lane, s1 = lane < NN - 64 ? lane + 64 : -100;       // -100: no entry that is compared equals it
    int n0 = 0, n1 = 0, w0 = 0, w1 = 0;                                // played and won_at of s0 and s1, this wave's playouts
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
        const int win = won[row0 + j0 + wave] != 0;
        const int16_t* row = rows[buf][wave];
        bool seen0 = false, seen1 = false, hit0 = false, hit1 = false;
        bool live = true;
        for (int k = 0; k < padded && live; k += 4) {
            const uint2 v = *reinterpret_cast<const uint2*>(row + k);
            const int m[4] = {(int16_t)(v.x & 0xFFFFu), (int16_t)(v.x >> 16), (int16_t)(v.y & 0xFFFFu), (int16_t)(v.y >> 16)};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                live = live && m[e] > BKT_MOVE_NONE;
                const bool mover = (e & 1) == 0;                       // ply k + e is even: k is a multiple of 4
                if (live && !seen0 && m[e] == s0) seen0 = true, hit0 = mover;
                if (live && !seen1 && m[e] == s1) seen1 = true, hit1 = mover;
            }
        }
        n0 += hit0, w0 += hit0 && win;
        n1 += hit1, w1 += hit1 && win;
    }
    part[wave][0][s0] = n0, part[wave][1][s0] = w0;
    if (s1 >= 0) part[wave][0][s1] = n1, part[wave][1][s1] = w1;
    __syncthreads();
    if (tid < NN) {
        int n = 0, w = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) n += part[v][0][tid], w += part[v][1][tid];
        played[(size_t)blockIdx.x * NN + tid] = n;
        won_at[(size_t)blockIdx.x * NN + tid] = w;
    }
}

}  // namespace

extern "C" int bkt_amaf_counts(const int16_t* moves, int max_plies, const uint8_t* won, int records, int playouts,
                               int32_t* played, int32_t* won_at, void* stream) {
    if (!moves || !won || !played || !won_at || records < 1 || playouts < 1 ||
        (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 || max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(amaf_counts_kernel, dim3(records), dim3(64 * WAVES), 0, (hipStream_t)stream, moves, max_plies, won,
                       playouts, played, won_at);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

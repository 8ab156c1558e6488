// bk_playout_nast_update.hip -- the update of a move-context table from a batch of playouts (NAST; include/bokego_train.h
// has the definition): bkt_move_context_update.  A translation unit of its own in libbktrain.so, beside
// bk_playout_mast_update.hip: it reads the move history the bkt_*_playouts calls write, the turn and the last move of the
// starting records and nothing else of theirs, and the text-include chain of bk_playout*.hip stays as it is.  The seating of
// the event pass is lgr2_events' (bk_playout_reply2.hip), repeated here on purpose.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int NN = 81;                       // points of the board
constexpr int PLANE = NN * NN;               // the offset of plane 81 within a colour
constexpr int COLOUR = (NN + 1) * NN;        // entries of a colour: 82 planes
constexpr int ENTRIES = 2 * COLOUR;          // 13,284 (colour, previous move, point)
constexpr int SINGLES = 2 * NN;              // the entries of plane 81: (colour, point)
constexpr int WAVES = 4;                     // waves of a workgroup of the event pass
constexpr int ROWS = 4;                      // rows a wave takes, one after the other
constexpr int POS_BYTES = 192;               // sizeof(bk_pos)
constexpr int OFF_KO = 164;                  // bk_pos.ko int16, then bk_pos.last_move int16 (bk_playout.hip asserts the layout)
constexpr int OFF_TURN = 172;                // bk_pos.turn, int32
constexpr size_t SCRATCH = (size_t)ENTRIES * 2 * sizeof(unsigned long long);   // 212,544 bytes: the call's (played, won) sums

__global__ void __launch_bounds__(256) ctxvalue_init_kernel(unsigned long long* __restrict__ sums) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < 2u * ENTRIES) sums[i] = 0ull;
}

// The event pass.  A wave per row, lanes over plies in chunks of 64; a wave takes ROWS rows one after the other and a
// workgroup WAVES * ROWS adjacent rows.  Lane j of chunk k0 looks at ply t = k0 + j: m = moves[t], p the move before (the
// record's last move at t = 0).  The row ends at the first m <= BKT_MOVE_NONE: the lowest set bit of a ballot, carried
// across chunks by leaving the loop -- wave-uniform, as the loop bounds are.  A ply with a board point m is a play of
// colour c = (colour to move at the record) xor (t & 1), won when (won[row] != 0) == (t even).  It always counts for
// plane 81: every play lands on one of those 162 entries, so they are summed per workgroup in LDS (uint32: a workgroup sees
// at most WAVES * ROWS * 1024 plays) and flushed behind the one barrier with a 64-bit atomic per non-zero field.  When p
// is a board point it counts for (c, p, m) too: 13,122 addresses, which take 64-bit atomic adds directly.  m and p are
// compared (0..80) before they index, so every entry is below ENTRIES.  Integer adds only: the sums do not depend on any
// order.  Every wave reaches the barrier: nothing returns before it.
__global__ void __launch_bounds__(64 * WAVES) ctxvalue_counts_kernel(const unsigned char* __restrict__ pos,
                                                                     const int16_t* __restrict__ moves, int max_plies,
                                                                     const uint8_t* __restrict__ won, long long rows,
                                                                     int playouts, unsigned long long* __restrict__ sums) {
    __shared__ unsigned singles[SINGLES][2];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < SINGLES) singles[tid][0] = 0u, singles[tid][1] = 0u;
    __syncthreads();
    const long long first_row = ((long long)blockIdx.x * WAVES + (tid >> 6)) * ROWS;
    for (int r = 0; r < ROWS; ++r) {
        const long long row = first_row + r;
        if (row >= rows) break;                                        // wave-uniform
        const unsigned char* rec = pos + (size_t)(row / playouts) * POS_BYTES;
        const int lm0 = (short)(*reinterpret_cast<const unsigned*>(rec + OFF_KO) >> 16);
        const int c0 = *reinterpret_cast<const int*>(rec + OFF_TURN) & 1;
        const bool win = won[row] != 0;
        const int16_t* src = moves + (size_t)row * max_plies;
        for (int k0 = 0; k0 < max_plies; k0 += 64) {
            const int t = k0 + lane;
            const int m = t < max_plies ? (int)src[t] : BKT_MOVE_NONE;
            const unsigned long long ends = __ballot(m <= BKT_MOVE_NONE);
            const int first = ends ? __ffsll((long long)ends) - 1 : 64;   // the lanes below it are the row's plies
            if (lane < first && m >= 0 && m < NN) {
                const int p = t == 0 ? lm0 : (int)src[t - 1];
                const int c = c0 ^ (t & 1);
                const bool mover_won = win == ((t & 1) == 0);
                atomicAdd(&singles[c * NN + m][0], 1u);
                if (mover_won) atomicAdd(&singles[c * NN + m][1], 1u);
                if (p >= 0 && p < NN) {
                    unsigned long long* at = sums + 2 * (size_t)(c * COLOUR + NN * p + m);
                    atomicAdd(at, 1ull);
                    if (mover_won) atomicAdd(at + 1, 1ull);
                }
            }
            if (ends) break;
        }
    }
    __syncthreads();
    if (tid < SINGLES) {
        const int c = tid / NN, m = tid - NN * c;
        unsigned long long* at = sums + 2 * (size_t)(c * COLOUR + PLANE + m);
        const unsigned n = singles[tid][0], w = singles[tid][1];
        if (n) atomicAdd(at, (unsigned long long)n);
        if (w) atomicAdd(at + 1, (unsigned long long)w);
    }
}

// The apply launch.  A workgroup per (colour, point): thread p < 82 owns the entry (c, p, m), adds the call's sums into
// counts, halves both fields until played < limit (limit > 0) and computes its index i = floor(64 (2 won + k) / (2 (played
// + k))), in 0..64 because won <= played.  Thread 81, the plane-81 entry, publishes its index i1 in LDS; behind the one
// barrier values[c][81][m] = lut[i1], and a context entry gets lut[(i1 + i) >> 1] when its played (after the shift) is at
// least min_plays, else lut[i1].  One writer per entry, no atomics; an index is compared before it indexes the lut.
__global__ void __launch_bounds__(128) ctxvalue_apply_kernel(const unsigned long long* __restrict__ sums,
                                                             int64_t* __restrict__ counts, uint16_t* __restrict__ values,
                                                             const uint16_t* __restrict__ lut, int k, int limit,
                                                             int min_plays) {
    __shared__ int plain;
    const int p = threadIdx.x;
    const int c = (int)blockIdx.x / NN, m = (int)blockIdx.x - NN * c;
    const int entry = c * COLOUR + NN * (p <= NN ? p : NN) + m;          // p > 81: thread 81's entry, read only
    unsigned long long played = (unsigned long long)counts[2 * entry] + sums[2 * entry];
    unsigned long long wins = (unsigned long long)counts[2 * entry + 1] + sums[2 * entry + 1];
    if (limit > 0)
        while (played >= (unsigned long long)limit) played >>= 1, wins >>= 1;
    const unsigned long long q = 64ull * (2ull * wins + (unsigned)k) / (2ull * (played + (unsigned)k));
    const int i = q < 64ull ? (int)q : 64;
    if (p == NN) plain = i;
    __syncthreads();
    if (p > NN) return;
    counts[2 * entry] = (int64_t)played, counts[2 * entry + 1] = (int64_t)wins;
    const int i1 = plain;
    values[entry] = lut[p < NN && played >= (unsigned long long)min_plays ? (i1 + i) >> 1 : i1];
}

}  // namespace

extern "C" size_t bkt_move_context_scratch_bytes(int records) { return records < 1 ? 0 : SCRATCH; }

extern "C" int bkt_move_context_update(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records,
                                       int playouts, int64_t* counts, uint16_t* values, const uint16_t* lut, int k, int limit,
                                       int min_plays, void* scratch, void* stream) {
    if (!pos || !moves || !won || !counts || !values || !lut || !scratch || records < 1 || playouts < 1 ||
        (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 || max_plies > BKT_MAX_PLAYOUT_PLIES ||
        (int64_t)playouts * max_plies >= (1ll << 31) || k < 1 || k > BKT_MOVE_VALUE_MAX_K ||
        (limit != 0 && (limit < 2 || limit > BKT_MOVE_VALUE_MAX_LIMIT)) || min_plays < 1 ||
        min_plays > BKT_MOVE_CONTEXT_MAX_MIN_PLAYS || (reinterpret_cast<uintptr_t>(counts) & 7u) ||
        (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return BKT_ERR_ARG;
    const long long rows = (long long)records * playouts;
    unsigned long long* sums = static_cast<unsigned long long*>(scratch);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ctxvalue_init_kernel, dim3((2 * ENTRIES + 255) / 256), dim3(256), 0, s, sums);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(ctxvalue_counts_kernel, dim3((unsigned)((rows + WAVES * ROWS - 1) / (WAVES * ROWS))), dim3(64 * WAVES), 0, s,
                       static_cast<const unsigned char*>(pos), moves, max_plies, won, rows, playouts, sums);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(ctxvalue_apply_kernel, dim3(SINGLES), dim3(128), 0, s, sums, counts, values, lut, k, limit, min_plays);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

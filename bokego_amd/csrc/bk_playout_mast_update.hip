// bk_playout_mast_update.hip -- the update of a move-value table from a batch of playouts (MAST; include/bokego_train.h has
// the definition): bkt_move_value_update.  A translation unit of its own in libbktrain.so, beside
// bk_playout_amaf.hip and bk_playout_rave.hip: it reads the move history the bkt_*_playouts calls write, the turn of the
// starting records and nothing else of theirs, and the text-include chain of bk_playout*.hip, whose kernels the resource
// tests pin, stays as it is.  The staging loop is amaf_counts_sides_kernel's, repeated here on purpose.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bokego_train.h"

namespace {

constexpr int NN = 81;                       // points of the board
constexpr int ENTRIES = 2 * NN;              // (colour, point)
constexpr int WAVES = 4;                     // rows staged per barrier round
constexpr int ROW = BKT_MAX_PLAYOUT_PLIES;   // int16 entries of a staged row (a multiple of 4: the scan reads 4 at a time)
constexpr int POS_BYTES = 192;               // sizeof(bk_pos)
constexpr int OFF_TURN = 172;                // bk_pos.turn, int32 (bk_playout.hip has the layout and asserts it)
constexpr int GROUP = 16;                    // entries of a workgroup of the second launch
constexpr int SLICES = 256 / GROUP;          // the records are dealt to this many threads per entry

// The first launch.  One workgroup per record r; thread t < 162 owns the entry (colour, point) = (t / 81, t % 81) and keeps
// its two counters in registers.  A round takes WAVES rows of the record:
//   stage  the whole workgroup copies their adjacent rows of `moves` into LDS, thread t the entries t, t + 256, ... of each
//          row (coalesced 2-byte loads), padded with BKT_MOVE_NONE to a multiple of 4 entries;
//   scan   after ONE barrier every thread walks the rows one after the other by 8-byte LDS reads at the same address in all
//          lanes (a broadcast), so the walk and its end at the first entry <= BKT_MOVE_NONE or at max_plies are uniform in
//          the workgroup.  Ply k + e with k a multiple of 4 has the parity of e, and the colour of its mover is the record's
//          colour to move xor that parity: a thread counts the plies of its own colour that carry its own point.
// Two LDS buffers alternate, so a round costs one barrier.  The record's partial counts go to scratch[r][played | won][162]
// by plain stores.  Integers only, no atomics; loop bounds and barriers depend on `playouts` and `max_plies` alone.  What is
// read: moves[row, k] for the record's rows and k < max_plies, won[row] for the same rows, four bytes of the record.  An
// entry is only compared, never used as an index: one above 80 matches no point, one below BKT_MOVE_NONE ends the row as
// that does.  A count is at most playouts * max_plies < 2^31 (the entry point's check).
__global__ void __launch_bounds__(64 * WAVES) movevalue_counts_kernel(const unsigned char* __restrict__ pos,
                                                                      const int16_t* __restrict__ moves, int max_plies,
                                                                      const uint8_t* __restrict__ won, int playouts,
                                                                      int32_t* __restrict__ scratch) {
    __shared__ __attribute__((aligned(8))) int16_t rows[2][WAVES][ROW];
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * playouts;                 // the record's first row
    const int padded = (max_plies + 3) & ~3;                           // <= ROW
    const int c0 = *reinterpret_cast<const int*>(pos + (size_t)blockIdx.x * POS_BYTES + OFF_TURN) & 1;
    const int my_c = tid / NN, mine = tid < ENTRIES ? tid - NN * my_c : -100;   // -100: no entry that is compared equals it
    const int my_e = my_c ^ c0;                                        // the parity of the plies of this thread's colour
    int n = 0, w = 0;
    int buf = 0;
    for (int j0 = 0; j0 < playouts; j0 += WAVES, buf ^= 1) {
        const int here = min(WAVES, playouts - j0);
        const int16_t* src = moves + (row0 + j0) * max_plies;
        for (int i = tid; i < padded; i += 64 * WAVES) {                // the round's loads first: WAVES in flight per thread
            int16_t e[WAVES];
#pragma unroll
            for (int v = 0; v < WAVES; ++v)
                e[v] = v < here && i < max_plies ? src[(size_t)v * max_plies + i] : (int16_t)BKT_MOVE_NONE;
#pragma unroll
            for (int v = 0; v < WAVES; ++v) rows[buf][v][i] = e[v];
        }
        __syncthreads();
        for (int v = 0; v < here; ++v) {                               // uniform in the workgroup
            const bool win = won[row0 + j0 + v] != 0;                  // the side to move at the record won the row
            const bool gain = win == (my_e == 0);                      // ... so this thread's colour did, or did not
            const int16_t* row = rows[buf][v];
            int hits = 0;
            bool live = true;
            for (int k = 0; k < padded && live; k += 4) {
                const uint2 x = *reinterpret_cast<const uint2*>(row + k);
                const int m[4] = {(int16_t)(x.x & 0xFFFFu), (int16_t)(x.x >> 16), (int16_t)(x.y & 0xFFFFu), (int16_t)(x.y >> 16)};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    live = live && m[e] > BKT_MOVE_NONE;
                    hits += live && m[e] == mine && (e & 1) == my_e;
                }
            }
            n += hits;
            w += gain ? hits : 0;
        }
    }
    if (tid < ENTRIES) {
        int32_t* out = scratch + (size_t)blockIdx.x * 2 * ENTRIES + tid;
        out[0] = n, out[ENTRIES] = w;
    }
}

// The second launch.  Workgroup g owns the entries 16 g .. 16 g + 15; thread t adds the partials of entry 16 g + t % 16 over
// the records t / 16, t / 16 + 16, ... (16 adjacent words per record and field), the 16 sums of an entry meet in LDS, and
// thread t < 16 adds them into counts, halves both fields until played < limit (limit > 0), and looks the value up:
// i = floor(64 (2 won + k) / (2 (played + k))), in 0..64 because won <= played.  One writer per entry, no atomics; the
// loop bound and the barrier depend on `records` alone.
__global__ void __launch_bounds__(256) movevalue_apply_kernel(const int32_t* __restrict__ scratch, int records,
                                                              int64_t* __restrict__ counts, uint16_t* __restrict__ values,
                                                              const uint16_t* __restrict__ lut, int k, int limit) {
    __shared__ unsigned long long part[2][SLICES][GROUP];
    const int tid = threadIdx.x, lane = tid % GROUP, slice = tid / GROUP;
    const int entry = (int)blockIdx.x * GROUP + lane;
    unsigned long long n = 0, w = 0;
    if (entry < ENTRIES)
        for (int r = slice; r < records; r += SLICES) {
            const int32_t* in = scratch + (size_t)r * 2 * ENTRIES + entry;
            n += (unsigned)in[0], w += (unsigned)in[ENTRIES];
        }
    part[0][slice][lane] = n, part[1][slice][lane] = w;
    __syncthreads();
    if (tid >= GROUP || entry >= ENTRIES) return;
    unsigned long long played = (unsigned long long)counts[2 * entry], wins = (unsigned long long)counts[2 * entry + 1];
#pragma unroll
    for (int s = 0; s < SLICES; ++s) played += part[0][s][tid], wins += part[1][s][tid];
    if (limit > 0)
        while (played >= (unsigned long long)limit) played >>= 1, wins >>= 1;
    counts[2 * entry] = (int64_t)played, counts[2 * entry + 1] = (int64_t)wins;
    const unsigned long long i = 64ull * (2ull * wins + (unsigned)k) / (2ull * (played + (unsigned)k));
    values[entry] = lut[i < 64ull ? (int)i : 64];                     // won <= played: i <= 64; compared before it indexes
}

}  // namespace

extern "C" size_t bkt_move_value_scratch_bytes(int records) {
    return records < 1 ? 0 : (size_t)records * 2 * ENTRIES * sizeof(int32_t);
}

extern "C" int bkt_move_value_update(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records,
                                     int playouts, int64_t* counts, uint16_t* values, const uint16_t* lut, int k, int limit,
                                     void* scratch, void* stream) {
    if (!pos || !moves || !won || !counts || !values || !lut || !scratch || records < 1 || playouts < 1 ||
        (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 || max_plies > BKT_MAX_PLAYOUT_PLIES ||
        (int64_t)playouts * max_plies >= (1ll << 31) || k < 1 || k > BKT_MOVE_VALUE_MAX_K ||
        (limit != 0 && (limit < 2 || limit > BKT_MOVE_VALUE_MAX_LIMIT)) || (reinterpret_cast<uintptr_t>(counts) & 7u) ||
        (reinterpret_cast<uintptr_t>(scratch) & 3u))
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(movevalue_counts_kernel, dim3(records), dim3(64 * WAVES), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), moves, max_plies, won, playouts, static_cast<int32_t*>(scratch));
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(movevalue_apply_kernel, dim3((ENTRIES + GROUP - 1) / GROUP), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const int32_t*>(scratch), records, counts, values, lut, k, limit);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

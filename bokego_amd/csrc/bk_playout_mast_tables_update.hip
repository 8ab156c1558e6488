// bk_playout_mast_tables_update.hip -- the update of a move-value table per game from a batch of playouts (include/
// bokego_train.h has the contract): bkt_move_value_update_tables.  A translation unit of its own in
// libbktrain.so, beside bk_playout_mast_update.hip, whose two kernels the tests pin and which stays as it is: the counts
// kernel is that file's, repeated here on purpose, and the apply kernel is its second launch with a
// table per workgroup column and the records' slots compared.
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

// The first launch: movevalue_counts_kernel of bk_playout_mast_update.hip, statement for statement.  One workgroup per
// record r, whatever its slot; thread t < 162 owns the entry (colour, point) = (t / 81, t % 81).  A round stages WAVES rows
// of the record in LDS (coalesced 2-byte loads, padded with BKT_MOVE_NONE to a multiple of 4 entries), and after ONE barrier
// every thread walks them by 8-byte LDS reads at the same address in all lanes, so the walk and its end are uniform in the
// workgroup.  Two LDS buffers alternate.  The record's partial counts go to scratch[r][played | won][162] by plain stores.
// Integers only, no atomics; loop bounds and barriers depend on `playouts` and `max_plies` alone.  What is read:
// moves[row, k] for the record's rows and k < max_plies, won[row] for the same rows, four bytes of the record.  An entry is
// only compared, never used as an index.  A count is at most playouts * max_plies < 2^31 (the entry point's check).
__global__ void __launch_bounds__(64 * WAVES) gamevalues_counts_kernel(const unsigned char* __restrict__ pos,
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

// The second launch, on a grid of (11, tables).  Workgroup (g, t) owns the entries 16 g .. 16 g + 15 of table t; thread x
// reads the slots of the records x / 16, x / 16 + 16, ... and adds the partials of entry 16 g + x % 16 of those whose slot
// is t (a slot that equals t is in range: it is compared, and indexes nothing).  Whether any record names the table is the
// barrier's own reduction; it is uniform in the workgroup, and a workgroup whose table no record names returns there and
// writes nothing.  Otherwise the 16 sums of an entry meet in LDS and thread x < 16 adds them into the table's counts,
// halves both fields until played < limit (limit > 0), and looks the value up, as the single-table kernel does.  One writer
// per entry, no atomics; the loop bound and the barrier depend on `records` alone.
__global__ void __launch_bounds__(256) gamevalues_apply_kernel(const int32_t* __restrict__ scratch, int records,
                                                               const int32_t* __restrict__ slots,
                                                               int64_t* __restrict__ counts, uint16_t* __restrict__ values,
                                                               const uint16_t* __restrict__ lut, int k, int limit) {
    __shared__ unsigned long long part[2][SLICES][GROUP];
    const int tid = threadIdx.x, lane = tid % GROUP, slice = tid / GROUP;
    const int entry = (int)blockIdx.x * GROUP + lane;
    const int t = (int)blockIdx.y;
    unsigned long long n = 0, w = 0;
    int named = 0;
    for (int r = slice; r < records; r += SLICES) {
        if (slots[r] != t) continue;
        named = 1;
        if (entry < ENTRIES) {
            const int32_t* in = scratch + (size_t)r * 2 * ENTRIES + entry;
            n += (unsigned)in[0], w += (unsigned)in[ENTRIES];
        }
    }
    part[0][slice][lane] = n, part[1][slice][lane] = w;
    if (!__syncthreads_or(named)) return;                             // uniform: no record names this table
    if (tid >= GROUP || entry >= ENTRIES) return;
    int64_t* const cnt = counts + (size_t)t * 2 * ENTRIES;
    unsigned long long played = (unsigned long long)cnt[2 * entry], wins = (unsigned long long)cnt[2 * entry + 1];
#pragma unroll
    for (int s = 0; s < SLICES; ++s) played += part[0][s][tid], wins += part[1][s][tid];
    if (limit > 0)
        while (played >= (unsigned long long)limit) played >>= 1, wins >>= 1;
    cnt[2 * entry] = (int64_t)played, cnt[2 * entry + 1] = (int64_t)wins;
    const unsigned long long i = 64ull * (2ull * wins + (unsigned)k) / (2ull * (played + (unsigned)k));
    values[(size_t)t * ENTRIES + entry] = lut[i < 64ull ? (int)i : 64];   // won <= played: i <= 64; compared before it indexes
}

}  // namespace

extern "C" size_t bkt_move_value_tables_scratch_bytes(int records, int tables) {
    return records < 1 || tables < 1 || tables > BKT_MAX_MOVE_VALUE_TABLES ? 0 : (size_t)records * 2 * ENTRIES * sizeof(int32_t);
}

extern "C" int bkt_move_value_update_tables(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won,
                                            int records, int playouts, int64_t* counts, uint16_t* values, const uint16_t* lut,
                                            int k, int limit, int tables, const int32_t* slots, void* scratch, void* stream) {
    if (!pos || !moves || !won || !counts || !values || !lut || !slots || !scratch || tables < 1 ||
        tables > BKT_MAX_MOVE_VALUE_TABLES || records < 1 || playouts < 1 ||
        (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 || max_plies > BKT_MAX_PLAYOUT_PLIES ||
        (int64_t)playouts * max_plies >= (1ll << 31) || k < 1 || k > BKT_MOVE_VALUE_MAX_K ||
        (limit != 0 && (limit < 2 || limit > BKT_MOVE_VALUE_MAX_LIMIT)) || (reinterpret_cast<uintptr_t>(counts) & 7u) ||
        (reinterpret_cast<uintptr_t>(scratch) & 3u))
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(gamevalues_counts_kernel, dim3(records), dim3(64 * WAVES), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), moves, max_plies, won, playouts, static_cast<int32_t*>(scratch));
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(gamevalues_apply_kernel, dim3((ENTRIES + GROUP - 1) / GROUP, tables), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const int32_t*>(scratch), records, slots, counts, values, lut, k, limit);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

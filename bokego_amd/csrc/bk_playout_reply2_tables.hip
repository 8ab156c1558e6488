// bk_playout_reply2_tables.hip -- included as text at the end of bk_playout_pat.hip, after bk_playout_reply2.hip (it is no
// translation unit of its own): a pair table per game of a self-play batch (include/bokego_train.h has the contract; DESIGN
// 27).  bkt_reply2_playouts_tables is bkt_reply2_playouts with the table of a row named by `slots`, as
// bkt_reply_playouts_tables names a single table; bkt_reply2_update_tables is bkt_reply2_update's event-parallel
// fold with the entry index offset by the record's slot.  The use rule and the update rule are DESIGN 26's.

namespace {

// The sixth draw.  Three pair tables do not fit in LDS at the tactical kernel's occupancy (3 x 13,284 bytes beside its 12,832
// leave no room for four workgroups a CU), so only plane 81 of a seat's table is staged, exactly as ReplyDraw<Inner, PPW>
// stages a single table (3 x 164 bytes, two rounds of the workgroup; 255 everywhere for a seat without a row or with a slot
// outside 0..tables-1 -- the slot is compared before it indexes), and in the first of a seat's two spare bytes whether the
// seat has a table at all.  The ply loop's first barrier publishes both.  The pair planes stay in global memory: every
// thread keeps the address of its row's table (table 0 for a row without one: an address that exists), resolved once in
// start(), where slots, tables, B and the kernel's table pointer are read for the last time.  Per ply a thread reads the
// one byte [c][lm2][lm] of that table, the same address in a whole row.  lm and lm2 are known at the top of publish() --
// L.mv holds the move just played and the inner draw the one before it -- so the load is issued there, before
// inner.publish()'s barriers, and its value is used only behind them.  Without a pair to ask, the address is the single
// entry [c][81][lm] again (entry 0 when lm is no board point; the result is then not used), so the load is unconditional.
// Nothing but integers in vector registers is carried across inner.publish(): a bool kept across it is a lane mask in two
// scalar registers, which this kernel does not have to spare, so what the lookup needs to know is asked again
// behind it.  Every entry is compared (<= 80) before it indexes L.playable.  No barrier is added.
template <class Inner>
struct GamePairsDraw {
    Inner inner;
    const uint8_t* __restrict__ replies2;
    const int32_t* __restrict__ slots;
    int tables, B;
    int q, reply, lm2;
    const uint8_t* mine2;                                            // this thread's row's table
    static constexpr int STRIDE = REPLY_ENTRIES + 2, HAS = REPLY_ENTRIES;
    static __device__ __forceinline__ uint8_t* lds() {
        __shared__ uint8_t table[PPW * STRIDE];
        return table;
    }
    __device__ __forceinline__ void start(Seat s, int last_move, int turn) {
        for (int i = s.tid; i < PPW * STRIDE; i += 256) {             // two rounds: 492 bytes
            const int seat = i / STRIDE, e = i - STRIDE * seat, c = e >= NN ? 1 : 0;
            const int row = (int)blockIdx.x * PPW + seat;
            const int slot = row < B ? slots[row] : -1;
            const bool has = slot >= 0 && slot < tables;
            const uint8_t r = replies2[(size_t)(has ? slot : 0) * REPLY2_ENTRIES + c * REPLY2_COLOUR + REPLY2_PLANE +
                                       (e < REPLY_ENTRIES ? e - NN * c : 0)];
            lds()[i] = e >= REPLY_ENTRIES ? (uint8_t)has : has ? r : (uint8_t)BKT_REPLY_NONE;
        }
        const int row = (int)blockIdx.x * PPW + s.pp;
        const int slot = row < B ? slots[row] : -1;
        mine2 = replies2 + (size_t)(slot >= 0 && slot < tables ? slot : 0) * REPLY2_ENTRIES;
        q = s.q, lm2 = REPLY2_NO_MOVE;
        inner.start(s, last_move, turn);
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B_, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B_, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds& L, bool mine, int played) {
        const int just = L.mv[s.pp];
        if (just > BKT_MOVE_NONE) lm2 = inner.lm;                    // a move was just played: the one before it moves on
        const int now = just > BKT_MOVE_NONE ? just : inner.lm;      // what inner.lm is behind inner.publish()
        const unsigned from = (((inner.turn0 + played) & 1) ? REPLY2_COLOUR : 0) +
                              (now >= 0 && now < NN ? (lm2 >= 0 && lm2 < NN ? NN * lm2 : REPLY2_PLANE) + now : REPLY2_PLANE);
        const uint8_t seen = mine2[from];                            // in flight across the inner draw's barriers
        inner.publish(s, L, mine, played);
        const int lm = inner.lm;
        const bool asks = lm >= 0 && lm < NN;
        const uint8_t* own = L.playable + NN * s.pp;
        const int r1 = lds()[STRIDE * s.pp + (((inner.turn0 + played) & 1) ? NN : 0) + (asks ? lm : 0)];
        const int r2 = lds()[STRIDE * s.pp + HAS] != 0 ? (int)seen : BKT_REPLY_NONE;
        const bool ok1 = asks && r1 < NN && own[r1 < NN ? r1 : 0] != 0, ok2 = asks && r2 < NN && own[r2 < NN ? r2 : 0] != 0;
        reply = ok2 ? r2 : ok1 ? r1 : -1;
    }
    __device__ __forceinline__ unsigned total(Seat s) { return inner.total(s); }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned S) const {
        return reply >= 0 ? q == reply : inner.picks(r24, S);
    }
};

__global__ void __launch_bounds__(256) gamepairs_weighted_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                 const uint32_t* __restrict__ counters,
                                                                 const uint16_t* __restrict__ table,
                                                                 const uint16_t* __restrict__ tactics,
                                                                 const uint8_t* __restrict__ replies2, int tables,
                                                                 const int32_t* __restrict__ slots, int max_plies,
                                                                 unsigned char* over, int32_t* __restrict__ plies,
                                                                 int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             GamePairsDraw<WeightedDraw<OptionalTacticalWeight>>{{{table, tactics}}, replies2, slots, tables, B});
}

__global__ void __launch_bounds__(256) gamepairs_uniform_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                const uint32_t* __restrict__ counters,
                                                                const uint8_t* __restrict__ replies2, int tables,
                                                                const int32_t* __restrict__ slots, int max_plies,
                                                                unsigned char* over, int32_t* __restrict__ plies,
                                                                int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ unsigned sel[8];
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             GamePairsDraw<TrackedUniformDraw>{{UniformDraw{sel}, 0, 0}, replies2, slots, tables, B});
}

// ---- the update ---------------------------------------------------------------------------------------------------------
// bkt_reply2_update's four launches over `tables` tables: entry e of table t is entry t * 13,284 + e of one long table, with
// a uint64 key per entry and, behind all keys, a flag byte per entry.  A wave of the two event passes is one row
// (lgr2_events' seating, used as it is): it reads its record's slot once, compares it, and raises its events at that
// offset, or none.  The order row * max_plies + ply, restricted to the records of one table, is that table's fold order, so
// the closed form holds per table; a table no record names has no key and no flag and keeps every byte.

__global__ void __launch_bounds__(256) gamepairs_init_kernel(uint32_t* __restrict__ scratch, unsigned dwords) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < dwords) scratch[i] = 0u;
}

// The offset of this wave's table in entries, or -1: no row, or a slot outside 0..tables-1.
__device__ __forceinline__ long long gamepairs_offset(const int32_t* __restrict__ slots, int tables, long long rows, int playouts) {
    const long long row = (long long)blockIdx.x * REPLY2_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return -1;
    const int slot = slots[row / playouts];
    return slot >= 0 && slot < tables ? (long long)slot * REPLY2_ENTRIES : -1;
}

__global__ void __launch_bounds__(64 * REPLY2_WAVES) gamepairs_store_kernel(const unsigned char* __restrict__ pos,
                                                                            const int16_t* __restrict__ moves, int max_plies,
                                                                            const uint8_t* __restrict__ won, long long rows,
                                                                            int playouts, int tables,
                                                                            const int32_t* __restrict__ slots,
                                                                            unsigned long long* __restrict__ keys) {
    const long long at = gamepairs_offset(slots, tables, rows, playouts);
    if (at < 0) return;                                              // wave-uniform; no barrier below
    lgr2_events(pos, moves, max_plies, won, rows, playouts, [=](int entry, unsigned long long order, int m, bool mover_won) {
        if (mover_won) atomicMax(keys + at + entry, (order + 1) << 8 | (unsigned long long)m);
    });
}

__global__ void __launch_bounds__(64 * REPLY2_WAVES) gamepairs_clear_kernel(const unsigned char* __restrict__ pos,
                                                                            const int16_t* __restrict__ moves, int max_plies,
                                                                            const uint8_t* __restrict__ won, long long rows,
                                                                            int playouts, int tables,
                                                                            const int32_t* __restrict__ slots,
                                                                            const unsigned long long* __restrict__ keys,
                                                                            const uint8_t* __restrict__ replies2,
                                                                            uint8_t* __restrict__ flags) {
    const long long at = gamepairs_offset(slots, tables, rows, playouts);
    if (at < 0) return;
    lgr2_events(pos, moves, max_plies, won, rows, playouts, [=](int entry, unsigned long long order, int m, bool mover_won) {
        if (mover_won) return;
        const unsigned long long key = keys[at + entry];
        const bool clears = key == 0 ? (int)replies2[at + entry] == m : order + 1 > key >> 8 && (int)(key & 255u) == m;
        if (clears) flags[at + entry] = 1;
    });
}

// One thread per (table, entry): it writes only where a flag or a key is set.
__global__ void __launch_bounds__(256) gamepairs_finish_kernel(const unsigned long long* __restrict__ keys,
                                                               const uint8_t* __restrict__ flags,
                                                               uint8_t* __restrict__ replies2, unsigned entries) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= entries) return;
    const unsigned long long key = keys[e];
    if (flags[e]) replies2[e] = (uint8_t)BKT_REPLY_NONE;
    else if (key) replies2[e] = (uint8_t)(key & 255u);
}

}  // namespace

extern "C" int bkt_reply2_playouts_tables(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                          const uint16_t* tactics, const uint8_t* replies2, int tables, const int32_t* slots,
                                          int max_plies, uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status,
                                          void* stream) {
    if (!replies2 || !reply2_aligned(replies2) || !slots || tables < 1 || tables > BKT_MAX_REPLY2_TABLES) return BKT_ERR_ARG;
    if (!table && !tactics)
        return launch_playouts(gamepairs_uniform_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status,
                               stream, replies2, tables, slots);
    return launch_playouts(gamepairs_weighted_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream,
                           table, tactics, replies2, tables, slots);
}

extern "C" size_t bkt_reply2_tables_scratch_bytes(int tables) {
    return tables < 1 || tables > BKT_MAX_REPLY2_TABLES ? 0 : (size_t)tables * REPLY2_SCRATCH;
}

extern "C" int bkt_reply2_update_tables(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records,
                                        int playouts, uint8_t* replies2, int tables, const int32_t* slots, void* scratch,
                                        void* stream) {
    if (!pos || !moves || !won || !replies2 || !slots || !scratch || !reply2_aligned(replies2) ||
        (reinterpret_cast<uintptr_t>(scratch) & 7u) || tables < 1 || tables > BKT_MAX_REPLY2_TABLES || records < 1 ||
        playouts < 1 || (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 || max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    const long long rows = (long long)records * playouts;
    const unsigned entries = (unsigned)tables * REPLY2_ENTRIES;      // <= 4096 * 13,284 < 2^26
    const unsigned dwords = (unsigned)((size_t)tables * REPLY2_SCRATCH / 4);
    const dim3 seats((unsigned)((rows + REPLY2_WAVES - 1) / REPLY2_WAVES));
    unsigned long long* keys = static_cast<unsigned long long*>(scratch);
    uint8_t* flags = static_cast<uint8_t*>(scratch) + (size_t)entries * sizeof(unsigned long long);
    const unsigned char* p = static_cast<const unsigned char*>(pos);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gamepairs_init_kernel, dim3((dwords + 255) / 256), dim3(256), 0, s, static_cast<uint32_t*>(scratch), dwords);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(gamepairs_store_kernel, seats, dim3(64 * REPLY2_WAVES), 0, s, p, moves, max_plies, won, rows, playouts,
                       tables, slots, keys);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(gamepairs_clear_kernel, seats, dim3(64 * REPLY2_WAVES), 0, s, p, moves, max_plies, won, rows, playouts,
                       tables, slots, keys, static_cast<const uint8_t*>(replies2), flags);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(gamepairs_finish_kernel, dim3((entries + 255) / 256), dim3(256), 0, s, keys, flags, replies2, entries);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

#include "bk_playout_mast.hip" // MAST playouts, a per-(colour, point) factor the playouts learn: text likewise

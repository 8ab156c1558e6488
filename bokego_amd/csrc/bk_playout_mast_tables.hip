// bk_playout_mast_tables.hip -- included as text at the end of bk_playout_mast.hip, and so at the end of bk_playout_pat.hip's
// chain (it is no translation unit of its own): a move-value table per game of a self-play batch (include/bokego_train.h
// has the contract).  bkt_move_value_playouts_tables is bkt_move_value_playouts with the table of a row named by
// `slots`, as bkt_reply_playouts_tables names a single reply table and bkt_reply2_playouts_tables a pair table
// (DESIGN 27); under either per-game reply draw the same slot names both tables of a row.  The weight rule is DESIGN 30's.
// The tables' update is a translation unit of its own, bk_playout_mast_tables_update.hip.

namespace {

// The Weight of the per-game move-value playouts: MoveValueWeight's with a table per seat.  stage() copies the 162 entries
// of each seat's row's table into LDS (PPW x 162 uint16, 972 bytes, two rounds of the workgroup; 256 everywhere for a seat
// without a row or with a slot outside 0..tables-1 -- the slot is compared before it indexes), published by the ply loop's
// first barrier: slots, tables, B and the pointer are read here for the last time.  operator() is MoveValueWeight's with
// the seat's offset in the LDS address: one read at 162 pp + 81 colour + q, the same 64-bit multiply and clamp.  No
// barrier, and no branch that is not the thread's own.
struct GameMoveValueWeight {
    OptionalTacticalWeight inner;
    const uint16_t* __restrict__ values;
    const int32_t* __restrict__ slots;
    int tables, B;
    static __device__ __forceinline__ uint16_t* lds() {
        __shared__ uint16_t table[PPW * MOVE_VALUE_ENTRIES];
        return table;
    }
    __device__ __forceinline__ void stage(int tid) const {
        inner.stage(tid);
        for (int i = tid; i < PPW * MOVE_VALUE_ENTRIES; i += 256) {   // two rounds: 486 entries
            const int seat = i / MOVE_VALUE_ENTRIES, e = i - MOVE_VALUE_ENTRIES * seat;
            const int row = (int)blockIdx.x * PPW + seat;
            const int slot = row < B ? slots[row] : -1;
            lds()[i] = slot >= 0 && slot < tables ? values[(size_t)slot * MOVE_VALUE_ENTRIES + e] : (uint16_t)256;
        }
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B_, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B_, over, L);
    }
    __device__ __forceinline__ unsigned operator()(const PatLds* W, int pp, int q, int lm, bool white_to_move) const {
        const unsigned w_in = inner(W, pp, q, lm, white_to_move);
        const uint64_t w = ((uint64_t)w_in * lds()[MOVE_VALUE_ENTRIES * pp + (white_to_move ? NN : 0) + q]) >> 8;
        return w > MOVE_VALUE_CAP ? MOVE_VALUE_CAP : w ? (unsigned)w : 1u;
    }
};

__global__ void __launch_bounds__(256) gamevalues_draw_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                              const uint32_t* __restrict__ counters,
                                                              const uint16_t* __restrict__ table,
                                                              const uint16_t* __restrict__ tactics,
                                                              const uint16_t* __restrict__ values, int tables,
                                                              const int32_t* __restrict__ slots, int max_plies,
                                                              unsigned char* over, int32_t* __restrict__ plies,
                                                              int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    MOVE_VALUE_PARK(plies, status);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             WeightedDraw<GameMoveValueWeight>{{{table, tactics}, values, slots, tables, B}});
}

__global__ void __launch_bounds__(256) gamevalues_single_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                const uint32_t* __restrict__ counters,
                                                                const uint16_t* __restrict__ table,
                                                                const uint16_t* __restrict__ tactics,
                                                                const uint16_t* __restrict__ values,
                                                                const uint8_t* __restrict__ replies, int tables,
                                                                const int32_t* __restrict__ slots, int max_plies,
                                                                unsigned char* over, int32_t* __restrict__ plies,
                                                                int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    MOVE_VALUE_PARK(plies, status);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<WeightedDraw<GameMoveValueWeight>, PPW>{{{{table, tactics}, values, slots, tables, B}}, replies, slots,
                                                               tables, B});
}

__global__ void __launch_bounds__(256) gamevalues_pairs_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                               const uint32_t* __restrict__ counters,
                                                               const uint16_t* __restrict__ table,
                                                               const uint16_t* __restrict__ tactics,
                                                               const uint16_t* __restrict__ values,
                                                               const uint8_t* __restrict__ replies2, int tables,
                                                               const int32_t* __restrict__ slots, int max_plies,
                                                               unsigned char* over, int32_t* __restrict__ plies,
                                                               int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    MOVE_VALUE_PARK(plies, status);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             GamePairsDraw<WeightedDraw<GameMoveValueWeight>>{{{{table, tactics}, values, slots, tables, B}}, replies2, slots,
                                                              tables, B});
}

}  // namespace

extern "C" int bkt_move_value_playouts_tables(void* pos, int batch, uint64_t seed, const uint32_t* counters,
                                              const uint16_t* table, const uint16_t* tactics, const uint16_t* values,
                                              const uint8_t* replies, const uint8_t* replies2, int tables, const int32_t* slots,
                                              int max_plies, uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status,
                                              void* stream) {
    if (!values || !slots || tables < 1 || tables > BKT_MAX_MOVE_VALUE_TABLES || (replies && replies2) ||
        (replies2 && !reply2_aligned(replies2)))
        return BKT_ERR_ARG;
    const auto launch = [&](auto kernel, auto... extra) {
        return launch_playouts(kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream, table, tactics,
                               values, extra..., tables, slots);
    };
    if (replies) return launch(gamevalues_single_kernel, replies);
    if (replies2) return launch(gamevalues_pairs_kernel, replies2);
    return launch(gamevalues_draw_kernel);
}

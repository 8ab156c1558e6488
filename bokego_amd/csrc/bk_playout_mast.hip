// bk_playout_mast.hip -- included as text at the end of bk_playout_reply2_tables.hip, and so at the end of bk_playout_pat.hip's
// chain (it is no translation unit of its own): MAST playouts, the move-average sampling technique of Finnsson & Bjornsson
// (include/bokego_train.h has the table and the two rules).  bkt_move_value_playouts is bkt_tactical_playouts
// whose weight is multiplied by a per-(colour, point) factor that the search's playouts learn, alone or under either reply
// draw.  The table's update is a translation unit of its own, bk_playout_mast_update.hip.

namespace {

constexpr int MOVE_VALUE_ENTRIES = 2 * NN;                           // values[colour][point]
constexpr unsigned MOVE_VALUE_CAP = (1u << 24) - 1u;                 // a weight stays below 2^24: a row's sum below 2^31

// The Weight of the move-value playouts: OptionalTacticalWeight's, times values[c][q] / 256.  stage() copies the 162
// entries into LDS beside the tactics table -- published by the ply loop's first barrier, as that one is -- so the pointer
// is dead in the loop.  operator() adds, behind tactical_weight's call, one LDS read (the colour to move picks the half,
// the thread's own point the entry) and one 64-bit multiply: w_in < 2^24 and an entry < 2^16, so the product needs 40
// bits.  No barrier, and no branch that is not the thread's own.
struct MoveValueWeight {
    OptionalTacticalWeight inner;
    const uint16_t* __restrict__ values;
    static __device__ __forceinline__ uint16_t* lds() {
        __shared__ uint16_t table[MOVE_VALUE_ENTRIES];
        return table;
    }
    __device__ __forceinline__ void stage(int tid) const {
        inner.stage(tid);
        if (tid < MOVE_VALUE_ENTRIES) lds()[tid] = values[tid];
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B, over, L);
    }
    __device__ __forceinline__ unsigned operator()(const PatLds* W, int pp, int q, int lm, bool white_to_move) const {
        const unsigned w_in = inner(W, pp, q, lm, white_to_move);
        const uint64_t w = ((uint64_t)w_in * lds()[(white_to_move ? NN : 0) + q]) >> 8;
        return w > MOVE_VALUE_CAP ? MOVE_VALUE_CAP : w ? (unsigned)w : 1u;
    }
};

// plies and status are written once, behind the ply loop: as scalars they would wait in SGPRs for its whole length, which the
// wrapped kernel already fills (105 of 106; the compiler spilled them).  Two vector registers each are free, and no
// instruction is emitted (bk_playout_balance.hip parks them the same way).
#define MOVE_VALUE_PARK(plies, status) asm volatile("" : "+v"(plies), "+v"(status))

__global__ void __launch_bounds__(256) movevalue_draw_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                             const uint32_t* __restrict__ counters,
                                                             const uint16_t* __restrict__ table,
                                                             const uint16_t* __restrict__ tactics,
                                                             const uint16_t* __restrict__ values, int max_plies,
                                                             unsigned char* over, int32_t* __restrict__ plies,
                                                             int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    MOVE_VALUE_PARK(plies, status);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             WeightedDraw<MoveValueWeight>{{{table, tactics}, values}});
}

__global__ void __launch_bounds__(256) movevalue_single_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                               const uint32_t* __restrict__ counters,
                                                               const uint16_t* __restrict__ table,
                                                               const uint16_t* __restrict__ tactics,
                                                               const uint16_t* __restrict__ values,
                                                               const uint8_t* __restrict__ replies, int max_plies,
                                                               unsigned char* over, int32_t* __restrict__ plies,
                                                               int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    MOVE_VALUE_PARK(plies, status);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<WeightedDraw<MoveValueWeight>, 1>{{{{table, tactics}, values}}, replies});
}

__global__ void __launch_bounds__(256) movevalue_pairs_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                              const uint32_t* __restrict__ counters,
                                                              const uint16_t* __restrict__ table,
                                                              const uint16_t* __restrict__ tactics,
                                                              const uint16_t* __restrict__ values,
                                                              const uint32_t* __restrict__ replies2, int max_plies,
                                                              unsigned char* over, int32_t* __restrict__ plies,
                                                              int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    MOVE_VALUE_PARK(plies, status);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             Reply2Draw<WeightedDraw<MoveValueWeight>>{{{{table, tactics}, values}}, replies2});
}

}  // namespace

extern "C" int bkt_move_value_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                       const uint16_t* tactics, const uint16_t* values, const uint8_t* replies,
                                       const uint8_t* replies2, int max_plies, uint8_t* over, int32_t* plies, int16_t* moves,
                                       int32_t* status, void* stream) {
    if (!values || (replies && replies2) || (replies2 && !reply2_aligned(replies2))) return BKT_ERR_ARG;
    const auto launch = [&](auto kernel, auto... extra) {
        return launch_playouts(kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream, table, tactics,
                               values, extra...);
    };
    if (replies) return launch(movevalue_single_kernel, replies);
    if (replies2) return launch(movevalue_pairs_kernel, reinterpret_cast<const uint32_t*>(replies2));
    return launch(movevalue_draw_kernel);
}

#include "bk_playout_mast_tables.hip" // a move-value table per game of a self-play batch: text likewise

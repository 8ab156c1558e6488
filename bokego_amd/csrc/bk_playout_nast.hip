// bk_playout_nast.hip -- included as text at the end of bk_playout_reply2.hip, and so inside bk_playout_pat.hip's chain (it
// is no translation unit of its own): NAST playouts, the N-gram average sampling technique of Powley, Whitehouse & Cowling
// and the N-gram selection of Tak, Winands & Bjornsson (include/bokego_train.h has the table and the two rules).
// bkt_move_context_playouts is bkt_tactical_playouts whose weight is multiplied by a factor keyed by (colour, previous move,
// point) that the search's playouts learn, alone or under either reply draw.  The table's update is a translation unit of
// its own, bk_playout_nast_update.hip.

namespace {

constexpr int CTXVALUE_COLOUR = (NN + 1) * NN;                       // values[c]: 82 planes of 81 entries
constexpr int CTXVALUE_ENTRIES = 2 * CTXVALUE_COLOUR;                // 13,284 uint16: 26,568 bytes, more than the LDS has room for
constexpr unsigned CTXVALUE_CAP = (1u << 24) - 1u;                   // a weight stays below 2^24: a row's sum below 2^31

// The Weight of the move-context playouts: OptionalTacticalWeight's, times values[c][p][q] / 256, p the move played just
// before (`lm`, which WeightedDraw carries: a pass, none or junk is plane 81 -- compared before it indexes).  The table does
// not fit beside the wrapped kernels' LDS at four workgroups a CU, so nothing is staged: a thread reads its one uint16 per
// ply from global memory (the table is read-only for the launch and 26.5 KB: it lives in L2).  The load is issued before
// tactical_weight's call, whose chain walks and pattern lookup it overlaps, and waited for behind it.  No barrier, no LDS,
// and no branch that is not the thread's own.
struct ContextValueWeight {
    OptionalTacticalWeight inner;
    const uint16_t* values;
    __device__ __forceinline__ void stage(int tid) const { inner.stage(tid); }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B, over, L);
    }
    __device__ __forceinline__ unsigned operator()(const PatLds* W, int pp, int q, int lm, bool white_to_move) const {
        const int p = lm >= 0 && lm < NN ? lm : NN;
        const unsigned v = values[(white_to_move ? CTXVALUE_COLOUR : 0) + NN * p + q];
        const unsigned w_in = inner(W, pp, q, lm, white_to_move);
        const uint64_t w = ((uint64_t)w_in * v) >> 8;
        return w > CTXVALUE_CAP ? CTXVALUE_CAP : w ? (unsigned)w : 1u;
    }
};

// plies and status are written once, behind the ply loop, and values is read in it by every thread at an address of its own:
// as scalars the three would wait in SGPRs for the loop's whole length, which the wrapped kernels already fill (the compiler
// spilled one and two of them under the reply draws).  Vector registers are free, and no instruction is emitted.
#define CTXVALUE_PARK(plies, status, values) asm volatile("" : "+v"(plies), "+v"(status), "+v"(values))

__global__ void __launch_bounds__(256) ctxvalue_draw_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                            const uint32_t* __restrict__ counters,
                                                            const uint16_t* __restrict__ table,
                                                            const uint16_t* __restrict__ tactics, const uint16_t* values,
                                                            int max_plies, unsigned char* over, int32_t* __restrict__ plies,
                                                            int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    CTXVALUE_PARK(plies, status, values);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             WeightedDraw<ContextValueWeight>{{{table, tactics}, values}});
}

__global__ void __launch_bounds__(256) ctxvalue_single_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                              const uint32_t* __restrict__ counters,
                                                              const uint16_t* __restrict__ table,
                                                              const uint16_t* __restrict__ tactics, const uint16_t* values,
                                                              const uint8_t* __restrict__ replies, int max_plies,
                                                              unsigned char* over, int32_t* __restrict__ plies,
                                                              int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    CTXVALUE_PARK(plies, status, values);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<WeightedDraw<ContextValueWeight>, 1>{{{{table, tactics}, values}}, replies});
}

__global__ void __launch_bounds__(256) ctxvalue_pairs_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                             const uint32_t* __restrict__ counters,
                                                             const uint16_t* __restrict__ table,
                                                             const uint16_t* __restrict__ tactics, const uint16_t* values,
                                                             const uint32_t* __restrict__ replies2, int max_plies,
                                                             unsigned char* over, int32_t* __restrict__ plies,
                                                             int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    CTXVALUE_PARK(plies, status, values);
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             Reply2Draw<WeightedDraw<ContextValueWeight>>{{{{table, tactics}, values}}, replies2});
}

}  // namespace

extern "C" int bkt_move_context_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                         const uint16_t* tactics, const uint16_t* values, const uint8_t* replies,
                                         const uint8_t* replies2, int max_plies, uint8_t* over, int32_t* plies, int16_t* moves,
                                         int32_t* status, void* stream) {
    if (!values || (replies && replies2) || (replies2 && !reply2_aligned(replies2))) return BKT_ERR_ARG;
    const auto launch = [&](auto kernel, auto... extra) {
        return launch_playouts(kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream, table, tactics,
                               values, extra...);
    };
    if (replies) return launch(ctxvalue_single_kernel, replies);
    if (replies2) return launch(ctxvalue_pairs_kernel, reinterpret_cast<const uint32_t*>(replies2));
    return launch(ctxvalue_draw_kernel);
}

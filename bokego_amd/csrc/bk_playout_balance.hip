// bk_playout_balance.hip -- included as text in bk_playout_pat.hip, after bk_playout_reply.hip, whose OptionalTacticalWeight it
// uses (it is no translation unit of its own): the gradient sums of simulation balancing (bokego_amd/balance.py;
// include/bokego_train.h has the definition).  bkt_balance_sums is bkt_tactical_playouts with either table
// optional, whose draw also books what the ply loop otherwise throws away: at every ply, every candidate's share of the draw,
// against the candidate's pattern index and tactical code.  BalanceDraw wraps WeightedDraw as ReplyDraw does; it reads the
// inner draw's registers (w, lm, turn0) and LDS (the stone ballots, the planes) and never changes a draw, so the games are
// those of the kernel it wraps.
//
// Accumulation: integer adds mod 2^64, so the sums do not depend on the order.  The lanes of a wave that hold the same
// (row, pattern index, tactical code) have the same weight and so the same share: they are counted, and one leader adds
// count x share; the picked point adds its 2^Q on its own.  The tactics sums and the 512 stone-free pattern indices --
// from the empty board nearly every point has one of them -- are kept in LDS and leave once per workgroup; the other pattern
// indices go to global memory by one 64-bit atomicAdd per leader.  Integers only; vector stores and vector atomics only.

namespace {

constexpr int BAL_Q = BKT_BALANCE_Q;
constexpr int BAL_HOT = 512;                                         // stone-free pattern indices, kept in LDS
static_assert(BAL_HOT == 2 * 256, "the workgroup clears and flushes the hot sums in two rounds");
typedef unsigned long long bal_u64;

// A pattern index whose eight neighbours are all empty or off the board (2-bit states 0 and 3 only), its slot among the 512
// of them (the even bits of the low 16, packed, | near << 8), and the slot's index again: bk_playout_mm.hip's three.
__device__ __forceinline__ bool bal_stone_free(unsigned i) { return ((i ^ (i >> 1)) & 0x5555u) == 0; }
__device__ __forceinline__ unsigned bal_hot_slot(unsigned i) {
    unsigned x = i & 0x5555u;
    x = (x | x >> 1) & 0x3333u, x = (x | x >> 2) & 0x0F0Fu, x = (x | x >> 4) & 0x00FFu;
    return x | (i >> 16 & 1u) << 8;
}
__device__ __forceinline__ unsigned bal_hot_index(unsigned slot) {
    unsigned x = slot & 0xFFu;
    x = (x | x << 4) & 0x0F0Fu, x = (x | x << 2) & 0x3333u, x = (x | x << 1) & 0x5555u;
    return x * 3u | (slot >> 8 & 1u) << 16;
}

struct BalLds {
    bal_u64 hot[BAL_HOT];
    bal_u64 dt[BKT_TACTIC_ENTRIES];
    bal_u64* grad_p;                                                 // the two accumulators: no pointer to keep in the loop
    bal_u64* grad_t;
};

// One add to both sums: idx < BKT_PATTERN_ENTRIES and code < BKT_TACTIC_ENTRIES, masked by the caller.
__device__ __forceinline__ void balance_add(BalLds* A, unsigned idx, unsigned code, bal_u64 add) {
    if (bal_stone_free(idx)) atomicAdd(&A->hot[bal_hot_slot(idx)], add);
    else atomicAdd(&A->grad_p[idx], add);
    atomicAdd(&A->dt[code], add);
}

// What the candidates of a ply book but for the picked point's 2^Q: -coef * floor(w 2^Q / S) each.  Called by the lanes of
// a wave that have something to book (w > 0, so S > 0, and coef != 0), whichever they are: the ballots see the calling lanes
// only, the leader is one of them, and the loop ends for all of them at once.  No barrier.  The pattern index and the
// tactical code are those tactical_weight made the point's weight from, out of the same ballots and planes, both masked to
// their tables (idx < 2^17, code < 64, the hot slot < 512), and pp < 3: the key is the (row, index, code).
// -> index | code << 17.  One call site, not inlined, as tactical_weight.
__device__ __noinline__ unsigned balance_book(BalLds* A, const PatLds* W, const TacLds* F, int pp, int q, int lm,
                                              bool white_to_move, unsigned w, unsigned S, int coef) {
    const BB black = position_set(W->bal[0], pp), white = position_set(W->bal[1], pp);
    const unsigned idx = pattern_index(white_to_move ? white : black, white_to_move ? black : white, q, lm) & (BKT_PATTERN_ENTRIES - 1);
    const unsigned code = tactic_code(F->planes + pp * PLANES_ROW, q) & (BKT_TACTIC_ENTRIES - 1);
    const bal_u64 share = ((bal_u64)w << BAL_Q) / S;                 // w < 2^24: the dividend is below 2^48; share <= 2^Q
    const unsigned word = idx | code << 17, key = word | (unsigned)pp << 23;
    const int lane = threadIdx.x & 63;
    bool waiting = true;
    for (bal_u64 rest = __ballot(waiting); rest; rest = __ballot(waiting)) {
        const int leader = __ffsll(rest) - 1;
        const bool mine = waiting && key == (unsigned)__shfl((int)key, leader);
        const long long n = __popcll(__ballot(mine));
        if (lane == leader) balance_add(A, idx, code, (bal_u64)(-(long long)coef * n * (long long)share));   // below 2^44
        waiting = waiting && !mine;
    }
    return word;
}

// The draw of bkt_balance_sums: the inner weighted draw, read and never changed.  start() clears the workgroup's sums in
// LDS and leaves the accumulators' addresses there (published by the ply loop's first barrier), and reads the row's
// coefficient; publish() is the inner one's and keeps the turn; total() is the inner one's, after which a playable point
// (w > 0) of a row with a coefficient books its share; picks() is the inner one's answer, and the picked point books its
// 2^Q.  Both come after the last barrier of the ply's draw; the branches on the coefficient, on w and on the pick are per
// thread and reach no barrier; the ballots and planes they read are written next by the following ply's play(), behind the
// loop's barrier.  The loop asks picks() only of a row that is not over and whose total is positive.
template <class Inner>
struct BalanceDraw {
    Inner inner;
    const int32_t* __restrict__ coefs;
    bal_u64* grad_p;
    bal_u64* grad_t;
    int coef, pp, q, turn;
    unsigned word;
    static __device__ __forceinline__ BalLds* lds() {
        __shared__ BalLds A;
        return &A;
    }
    __device__ __forceinline__ void start(Seat s, int last_move, int turn0) {
        BalLds* const A = lds();
        A->hot[s.tid] = 0, A->hot[s.tid + 256] = 0;                   // BAL_HOT: two rounds of the workgroup
        if (s.tid < BKT_TACTIC_ENTRIES) A->dt[s.tid] = 0;
        if (s.tid == 0) A->grad_p = grad_p, A->grad_t = grad_t;
        coef = s.live ? coefs[(size_t)blockIdx.x * PPW + s.p] : 0;   // live: the row exists
        pp = s.pp, q = s.q, turn = turn0, word = 0;
        inner.start(s, last_move, turn0);
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds& L, bool mine, int played) {
        inner.publish(s, L, mine, played);
        turn = inner.turn0 + played;
    }
    __device__ __forceinline__ unsigned total(Seat s) {
        const unsigned S = inner.total(s);
        if (coef != 0 && inner.w != 0)
            word = balance_book(lds(), Inner::lds(), TacticalWeight::lds(), pp, q, inner.lm, (turn & 1) != 0, inner.w, S, coef);
        return S;
    }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned S) const {
        const bool hit = inner.picks(r24, S);                        // w > 0 where it is true: `word` is this ply's
        if (hit && coef != 0)
            balance_add(lds(), word & (BKT_PATTERN_ENTRIES - 1), word >> 17 & (BKT_TACTIC_ENTRIES - 1),
                        (bal_u64)((long long)coef << BAL_Q));
        return hit;
    }
};

__global__ void __launch_bounds__(256) balance_sums_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                           const uint32_t* __restrict__ counters,
                                                           const uint16_t* __restrict__ table,
                                                           const uint16_t* __restrict__ tactics,
                                                           const int32_t* __restrict__ coef, bal_u64* __restrict__ grad_p,
                                                           bal_u64* __restrict__ grad_t, int max_plies, unsigned char* over,
                                                           int32_t* __restrict__ plies, int16_t* __restrict__ hist,
                                                           int32_t* __restrict__ status) {
    using Draw = BalanceDraw<WeightedDraw<OptionalTacticalWeight>>;
    // plies and status are written once, behind the loop: as scalars they would wait in SGPRs for its whole length, which the
    // wrapped kernel already fills (the compiler spilled them); two vector registers each are free (no instruction is emitted)
    asm volatile("" : "+v"(plies), "+v"(status));
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status, Draw{{{table, tactics}}, coef, grad_p, grad_t});
    __syncthreads();                                                 // every thread: the ply loop's exit is workgroup-uniform
    const BalLds* const A = Draw::lds();
#pragma unroll
    for (int i = threadIdx.x; i < BAL_HOT; i += 256)                 // two rounds
        if (A->hot[i]) atomicAdd(&A->grad_p[bal_hot_index(i)], A->hot[i]);
    if (threadIdx.x < BKT_TACTIC_ENTRIES && A->dt[threadIdx.x]) atomicAdd(&A->grad_t[threadIdx.x], A->dt[threadIdx.x]);
}

}  // namespace

extern "C" int bkt_balance_sums(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                const uint16_t* tactics, const int32_t* coef, int64_t* grad_p, int64_t* grad_t, int max_plies,
                                uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status, void* stream) {
    if (!coef || !grad_p || !grad_t || batch > BKT_BALANCE_MAX_ROWS) return BKT_ERR_ARG;
    return launch_playouts(balance_sums_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream, table,
                           tactics, coef, reinterpret_cast<bal_u64*>(grad_p), reinterpret_cast<bal_u64*>(grad_t));
}

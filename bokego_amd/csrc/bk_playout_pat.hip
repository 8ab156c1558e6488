// bk_playout_pat.hip -- the translation unit of the device Go rules in libbktrain.so: bk_playout_mc.hip as it is (textually,
// and through it bk_playout.hip, so that both still compile alone for the resource tests that pin their kernels), and
// appended after them the pattern-weighted playouts of bokego_amd/patterns.py (include/bokego_train.h):
// bkt_pattern_codes, the 3x3 pattern index of every point of a record, and bkt_pattern_playouts, the ply loop of
// bk_playout_mc.hip with the weighted draw (WeightedDraw).  bk_playout_tac.hip, included as text at the end, gives that
// draw another weight: the tactical playouts.
//
// The index of a point s = 9r + c, relative to the side to move: the eight neighbours in the order (-1,0) (+1,0) (0,-1)
// (0,+1) (-1,-1) (-1,+1) (+1,-1) (+1,+1) give two bits each (0 empty, 1 the mover's stone, 2 the opponent's, 3 off the
// board), slot i at bit 2i; bit 16 is `near`: the record's last move is a board point at most one step away (itself
// included).  A table is uint16[131072]; the weight of a point is max(entry, 1).
#include "bk_playout_mc.hip"

namespace {

constexpr int PAT_ROW = 84;                                          // 81 weights and three zeros: 21 uint4

__device__ __forceinline__ unsigned neighbour_state(BB mine, BB theirs, int r, int c) {
    if (r < 0 || r >= 9 || c < 0 || c >= 9) return 3u;
    const BB m = point(9 * r + c);
    return meets(mine, m) ? 1u : meets(theirs, m) ? 2u : 0u;
}

__device__ __forceinline__ unsigned pattern_index(BB mine, BB theirs, int q, int lm) {
    const int r = q / 9, c = q - 9 * r;
    unsigned idx = neighbour_state(mine, theirs, r - 1, c) | neighbour_state(mine, theirs, r + 1, c) << 2 |
                   neighbour_state(mine, theirs, r, c - 1) << 4 | neighbour_state(mine, theirs, r, c + 1) << 6 |
                   neighbour_state(mine, theirs, r - 1, c - 1) << 8 | neighbour_state(mine, theirs, r - 1, c + 1) << 10 |
                   neighbour_state(mine, theirs, r + 1, c - 1) << 12 | neighbour_state(mine, theirs, r + 1, c + 1) << 14;
    if (lm >= 0 && lm < NN) {
        const int rl = lm / 9, dr = r - rl, dc = c - (lm - 9 * rl);
        if (dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1) idx |= 1u << 16;
    }
    return idx;
}

struct PatLds {
    unsigned bal[2][8];                                              // black / white ballots of the 4 waves
    __align__(16) unsigned w[PPW][PAT_ROW];                          // the weights of a row's points, 0 outside P
};

// max(table[index of point q of row pp], 1) from the row's stone ballots.  One call site, not inlined, as play_one_ply:
// inlined into the ply loop, the point's loop-invariant neighbour masks are hoisted out of it and stay live across the body.
__device__ __noinline__ unsigned point_weight(const PatLds* W, const uint16_t* __restrict__ table, int pp, int q, int lm,
                                              bool white_to_move) {
    const BB black = position_set(W->bal[0], pp), white = position_set(W->bal[1], pp);
    const unsigned w = table[pattern_index(white_to_move ? white : black, white_to_move ? black : white, q, lm)];
    return w ? w : 1u;
}

__global__ void __launch_bounds__(256) pattern_codes_kernel(const unsigned char* __restrict__ pos, int B,
                                                            int32_t* __restrict__ codes) {
    __shared__ unsigned bal[2][8];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    const int pp = p < PPW ? p : 0;
    int stone = 0, lm = BK_NO_MOVE, turn = 0;
    if (live) {
        const unsigned char* rec = pos + (size_t)(b0 + p) * BK_POS_BYTES;
        stone = (signed char)rec[q];
        lm = (short)(*reinterpret_cast<const unsigned*>(rec + OFF_KO) >> 16);
        turn = *reinterpret_cast<const int*>(rec + OFF_TURN);
    }
    publish_ballots(bal, tid, stone == BK_BLACK, stone == BK_WHITE);
    __syncthreads();
    if (!live) return;
    const BB black = position_set(bal[0], pp), white = position_set(bal[1], pp);
    const bool wtm = (turn & 1) != 0;
    codes[(size_t)(b0 + p) * NN + q] = (int32_t)pattern_index(wtm ? white : black, wtm ? black : white, q, lm);
}

// The weighted draw.  Per ply, after play_body<true> has left the playable set P in LDS: every thread reads its own board
// byte back (it wrote it itself), two ballots give the stone sets, a playable point asks `weight` for its weight and all
// of a row's weights go to LDS (0 outside P); after one barrier every thread sums the row's entries below its own point and
// the whole row, S; t = (r24 * S) >> 24, and the move is the point whose interval [below, below + w) holds t -- exactly
// one, since t < S.  The side to move and the last move are carried in registers (the parity flips with every ply played;
// the move just played is still in L.mv), so nothing is read that another thread wrote to global memory.  A Weight is
// the weight of a point, w < 2^24, what it stages in LDS before the loop, and the draw's play().
template <class Weight>
struct WeightedDraw {
    Weight weight;
    int lm, turn0;
    unsigned w, below;
    static __device__ __forceinline__ PatLds* lds() {                // a constant to the compiler, which a member is not
        __shared__ PatLds W;
        return &W;
    }
    __device__ __forceinline__ void start(Seat s, int last_move, int turn) {
        PatLds* const W = lds();
        lm = last_move, turn0 = turn;
        if (s.p < PPW && s.q < PAT_ROW - NN) W->w[s.p][NN + s.q] = 0;
        weight.stage(s.tid);
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        weight.play(pos, B, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds& L, bool mine, int played) {
        PatLds* const W = lds();
        const int stone = s.live ? (signed char)s.rec[s.q] : 0;      // this thread's own store
        publish_ballots(W->bal, s.tid, stone == BK_BLACK, stone == BK_WHITE);
        const int just = L.mv[s.pp];                                 // the move the body has just played, if any
        if (just > BKT_MOVE_NONE) lm = just;
        __syncthreads();
        w = 0;
        if (mine) w = weight(W, s.pp, s.q, lm, ((turn0 + played) & 1) != 0);
        if (s.p < PPW) W->w[s.p][s.q] = w;
        __syncthreads();
    }
    __device__ __forceinline__ unsigned total(Seat s) {
        unsigned S = 0;                                              // S <= 81 * (2^24 - 1) < 2^31
        below = 0;
        const uint4* row = reinterpret_cast<const uint4*>(lds()->w[s.pp]);
#pragma unroll 1                                                     // unrolled, the 84 loop-invariant compares fill the SGPRs
        for (int j = 0; j < PAT_ROW / 4; ++j) {
            const uint4 v = row[j];
            S += v.x + v.y + v.z + v.w;
            below += (4 * j < s.q ? v.x : 0u) + (4 * j + 1 < s.q ? v.y : 0u) + (4 * j + 2 < s.q ? v.z : 0u) +
                     (4 * j + 3 < s.q ? v.w : 0u);
        }
        return S;
    }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned S) const {
        const unsigned t = (unsigned)(((uint64_t)r24 * S) >> 24);    // 24 x 31 bits: 64-bit product; t < S
        return below <= t && t - below < w;
    }
};

// The pattern weight, max(table entry, 1) <= 65535: S <= 81 * 65535 < 2^23.
struct PatternWeight {
    const uint16_t* __restrict__ table;
    __device__ __forceinline__ void stage(int) const {}
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        play_one_ply(pos, B, over, L);
    }
    __device__ __forceinline__ unsigned operator()(const PatLds* W, int pp, int q, int lm, bool white_to_move) const {
        return point_weight(W, table, pp, q, lm, white_to_move);
    }
};

__global__ void __launch_bounds__(256) pattern_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                               const uint32_t* __restrict__ counters,
                                                               const uint16_t* __restrict__ table, int max_plies,
                                                               unsigned char* over, int32_t* __restrict__ plies,
                                                               int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status, WeightedDraw<PatternWeight>{{table}});
}

// The argument check and the launch of the bkt_*_codes entry points.
template <class Pos>
int launch_codes(void (*kernel)(Pos*, int, int32_t*), const void* pos, int batch, int32_t* codes, void* stream) {
    if (!pos || !codes || batch < 1 || batch > BKT_MAX_BATCH) return BKT_ERR_ARG;
    hipLaunchKernelGGL(kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<Pos*>(const_cast<void*>(pos)), batch, codes);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

}  // namespace

extern "C" int bkt_pattern_codes(const void* pos, int batch, int32_t* codes, void* stream) {
    return launch_codes(pattern_codes_kernel, pos, batch, codes, stream);
}

extern "C" int bkt_pattern_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                    int max_plies, uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status,
                                    void* stream) {
    if (!table) return BKT_ERR_ARG;
    return launch_playouts(pattern_playouts_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream,
                           table);
}

#include "bk_playout_tac.hip"   // the tactical playouts: text, part of this translation unit
#include "bk_playout_reply.hip" // the last-good-reply playouts and their table's update: text likewise
#include "bk_playout_balance.hip" // the gradient sums of simulation balancing: likewise
#include "bk_playout_reply2.hip" // replies keyed by the last two moves and their event-parallel update: likewise
#include "bk_playout_reply2_tables.hip" // a pair table per game of a self-play batch: likewise

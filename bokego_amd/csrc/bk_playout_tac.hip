// bk_playout_tac.hip -- included as text at the end of bk_playout_pat.hip (it is no translation unit of its own): the
// tactical playouts of bokego_amd/tactics.py (include/bokego_train.h): bkt_tactical_codes, the tactical code of
// every point of a record, and bkt_tactical_playouts, bkt_pattern_playouts whose weights are multiplied by a second table
// indexed by that code: the weighted draw of bk_playout_pat.hip with TacticalWeight.
//
// The code of a point q is read off the 27 planes F that play_body<true> computes on every ply anyway (bk_enc::
// encode_points on the updated record; the sibling kernels pass planes = nullptr and throw them away):
//   cap = planes 20..26 at q (stones captured by playing q), C = min(cap, 3);
//   la  = planes 13..19 at q (liberties after playing q; 0: not legal), A = 0 for la <= 1, 1 for la == 2, 2 for la >= 3;
//   E   = some on-board 4-neighbour t has F[0][t] && F[6][t]: a stone of the side to move whose cached liberty count is 1;
//   G   = some on-board 4-neighbour t has F[1][t] && F[7][t]: an opponent stone whose cached liberty count is 2;
//   code = C | A << 2 | E << 4 | G << 5, in [0, BKT_TACTIC_ENTRIES).
// The liberty planes are the reference's cache and can be stale; the code is a function of the record's bytes all the same.
//
// The tactical playouts need one more LDS buffer, the planes of the workgroup's three rows (PPW * 2187 bytes), which
// play_body fills through its `planes` argument (shifted by -b0 rows as the other per-row arguments).  The barrier that
// publishes the playable set publishes the planes too; a playable point then reads its own la and cap and its neighbours'
// planes 0, 1, 6 and 7, and its weight is w = max(1, (P * T) >> 8) with P the pattern weight (256 without a pattern table)
// and T = tactics[code]: w <= 65535^2 >> 8 < 2^24.  A tactics table of 256 everywhere gives w = P: bkt_pattern_playouts'
// games, or with no pattern table a constant weight: bkt_random_playouts' games.

namespace {

constexpr int PLANES_ROW = 27 * NN;                                  // the planes of one record: [27][81] bytes

struct TacLds {
    __align__(16) unsigned char planes[PPW * PLANES_ROW];
    uint16_t tactics[BKT_TACTIC_ENTRIES];                            // the table, staged once: no pointer to keep in the loop
};

// play_one_ply with the planes kept.  One call site per kernel, not inlined, for play_one_ply's reason.
__device__ __noinline__ void play_one_ply_planes(unsigned char* pos, int B, unsigned char* over, PlyLds* L, TacLds* F) {
    const int b0 = blockIdx.x * PPW;
    play_body<true>(pos, L->mv - b0, B, over, L->st - b0, F->planes - (size_t)b0 * PLANES_ROW, L->playable - (size_t)b0 * NN);
}

// The code of point q from the planes F of its record.  At most one of planes 13..19 and one of 20..26 is non-zero at q.
__device__ __forceinline__ unsigned tactic_code(const unsigned char* F, int q) {
    unsigned la = 0, cap = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        la |= F[(13 + i) * NN + q];
        cap |= F[(20 + i) * NN + q];
    }
    const int r = q / 9, c = q - 9 * r;
    const int nbr[4] = {q + 9, q - 9, q + 1, q - 1};
    const bool nv[4] = {r + 1 < 9, r >= 1, c + 1 < 9, c >= 1};
    unsigned e = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = nv[j] ? nbr[j] : q;                            // off the board: the point itself, and not counted
        const unsigned own1 = F[t] && F[6 * NN + t], opp2 = F[NN + t] && F[7 * NN + t];
        if (nv[j]) { e |= own1; g |= opp2; }
    }
    return (cap < 3u ? cap : 3u) | (la <= 1u ? 0u : la == 2u ? 1u : 2u) << 2 | e << 4 | g << 5;
}

// w = max(1, (P * T) >> 8) < 2^24 of point q of row pp: P = max(table[pattern index], 1), or 256 without a table;
// T = F->tactics[code].  One call site, not inlined, as point_weight.
__device__ __noinline__ unsigned tactical_weight(const PatLds* W, const TacLds* F, const uint16_t* __restrict__ table,
                                                 int pp, int q, int lm, bool white_to_move) {
    unsigned P = 256u;
    if (table) {
        const BB black = position_set(W->bal[0], pp), white = position_set(W->bal[1], pp);
        P = table[pattern_index(white_to_move ? white : black, white_to_move ? black : white, q, lm)];
        P = P ? P : 1u;
    }
    const unsigned w = (P * (unsigned)F->tactics[tactic_code(F->planes + pp * PLANES_ROW, q)]) >> 8;   // < 2^32 before the shift
    return w ? w : 1u;
}

__global__ void __launch_bounds__(256) tactical_codes_kernel(unsigned char* pos, int B, int32_t* __restrict__ codes) {
    __shared__ PlyLds L;
    __shared__ TacLds F;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    if (live && q == 0) L.mv[p] = BKT_MOVE_NONE;                     // no move: an untouched record, and its planes
    __syncthreads();
    play_one_ply_planes(pos, B, nullptr, &L, &F);
    __syncthreads();
    if (live) codes[(size_t)(b0 + p) * NN + q] = (int32_t)tactic_code(F.planes + p * PLANES_ROW, q);
}

// The Weight of the tactical playouts: the table staged in LDS once, the planes kept on every ply, tactical_weight.
struct TacticalWeight {
    const uint16_t* __restrict__ table;
    const uint16_t* __restrict__ tactics;
    static __device__ __forceinline__ TacLds* lds() {                // as WeightedDraw::lds
        __shared__ TacLds F;
        return &F;
    }
    __device__ __forceinline__ void stage(int tid) const {
        if (tid < BKT_TACTIC_ENTRIES) lds()->tactics[tid] = tactics[tid];   // published by the loop's first barrier
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        play_one_ply_planes(pos, B, over, L, lds());
    }
    __device__ __forceinline__ unsigned operator()(const PatLds* W, int pp, int q, int lm, bool white_to_move) const {
        return tactical_weight(W, lds(), table, pp, q, lm, white_to_move);
    }
};

__global__ void __launch_bounds__(256) tactical_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                const uint32_t* __restrict__ counters,
                                                                const uint16_t* __restrict__ table,
                                                                const uint16_t* __restrict__ tactics, int max_plies,
                                                                unsigned char* over, int32_t* __restrict__ plies,
                                                                int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status, WeightedDraw<TacticalWeight>{{table, tactics}});
}

}  // namespace

extern "C" int bkt_tactical_codes(const void* pos, int batch, int32_t* codes, void* stream) {
    // the ply body takes records it may play on; with BKT_MOVE_NONE for every row it only reads them
    return launch_codes(tactical_codes_kernel, pos, batch, codes, stream);
}

extern "C" int bkt_tactical_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                     const uint16_t* tactics, int max_plies, uint8_t* over, int32_t* plies, int16_t* moves,
                                     int32_t* status, void* stream) {
    if (!tactics) return BKT_ERR_ARG;
    return launch_playouts(tactical_playouts_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream,
                           table, tactics);
}

// bk_playout_tac.hip -- included as text at the end of bk_playout_pat.hip (it is no translation unit of its own): the
// tactical playouts of bokego_amd/tactics.py (include/bokego_train.h): bkt_tactical_codes, the tactical code of
// every point of a record, and bkt_tactical_playouts, bkt_pattern_playouts whose weights are multiplied by a second table
// indexed by that code.
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
// tactical_playouts_kernel is pattern_playouts_kernel with one more LDS buffer, the planes of the workgroup's three rows
// (PPW * 2187 bytes), which play_body fills through its `planes` argument (shifted by -b0 rows as the other per-row
// arguments).  The barrier that publishes the playable set publishes the planes too; a playable point then reads its own
// la and cap and its neighbours' planes 0, 1, 6 and 7, and its weight is w = max(1, (P * T) >> 8) with P the pattern weight
// (256 without a pattern table) and T = tactics[code]: w <= 65535^2 >> 8 < 2^24, a row's sum S <= 81 * 2^24 < 2^31, and
// the draw is the siblings': t = ((x0 >> 8) * S) >> 24 in 64 bits, the point whose interval [below, below + w) holds t.
// A tactics table of 256 everywhere gives w = P: bkt_pattern_playouts' games, or with no pattern table a constant weight:
// bkt_random_playouts' games.  All barriers and the exit test are workgroup-uniform; nothing crosses workgroups; no
// atomics, no spinning; integer work and plain vector stores.

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

// max(1, (P * T) >> 8) of point q of row pp: P = max(table[pattern index], 1), or 256 without a table; T = F->tactics[code].
// One call site, not inlined, as point_weight.
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

__global__ void __launch_bounds__(256) tactical_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                const uint32_t* __restrict__ counters,
                                                                const uint16_t* __restrict__ table,
                                                                const uint16_t* __restrict__ tactics, int max_plies,
                                                                unsigned char* over, int32_t* __restrict__ plies,
                                                                int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ PlyLds L;
    __shared__ PatLds W;
    __shared__ TacLds F;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    const int pp = p < PPW ? p : 0;
    const int b = b0 + (live ? p : 0);
    bool done = true, last_pass = false;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    int lm = BK_NO_MOVE, turn0 = 0;
    if (live) {
        done = over[b] != 0;
        lm = (short)(*reinterpret_cast<const unsigned*>(pos + (size_t)b * BK_POS_BYTES + OFF_KO) >> 16);
        turn0 = *reinterpret_cast<const int*>(pos + (size_t)b * BK_POS_BYTES + OFF_TURN);
        last_pass = lm == BK_PASS;
        c0 = counters[4 * (size_t)b], c1 = counters[4 * (size_t)b + 1];
        c2 = counters[4 * (size_t)b + 2], c3 = counters[4 * (size_t)b + 3];
        if (q == 0) L.mv[p] = BKT_MOVE_NONE;
    }
    if (p < PPW && q < PAT_ROW - NN) W.w[p][NN + q] = 0;
    if (tid < BKT_TACTIC_ENTRIES) F.tactics[tid] = tactics[tid];     // published by the loop's first barrier
    int16_t* const hrow = hist ? hist + (size_t)b * max_plies : nullptr;
    int played = 0, st_or = 0, ply = 0;
    for (;; ++ply) {                                                 // round `ply` selects ply `ply`; the body before it
        __syncthreads();                                             // plays ply `ply - 1` (round 0: no move, the start sets)
        play_one_ply_planes(pos, B, over, &L, &F);
        if (live && q == 0) st_or |= L.st[p];
        if (ply == max_plies) break;
        if (!__syncthreads_or(live && !done)) break;                 // (the barrier also publishes L.playable and F.planes)
        const bool mine = live && !done && L.playable[NN * pp + q] != 0;
        const int stone = live ? (signed char)pos[(size_t)b * BK_POS_BYTES + q] : 0;   // this thread's own store
        publish_ballots(W.bal, tid, stone == BK_BLACK, stone == BK_WHITE);
        const int just = L.mv[pp];                                   // the move the body has just played, if any
        if (just > BKT_MOVE_NONE) lm = just;
        __syncthreads();
        unsigned w = 0;
        if (mine) w = tactical_weight(&W, &F, table, pp, q, lm, ((turn0 + played) & 1) != 0);
        if (p < PPW) W.w[p][q] = w;
        __syncthreads();
        if (live) {
            unsigned S = 0, below = 0;                               // S <= 81 * (2^24 - 1) < 2^31
            const uint4* row = reinterpret_cast<const uint4*>(W.w[pp]);
#pragma unroll 1                                                     // as pattern_playouts_kernel
            for (int j = 0; j < PAT_ROW / 4; ++j) {
                const uint4 v = row[j];
                S += v.x + v.y + v.z + v.w;
                below += (4 * j < q ? v.x : 0u) + (4 * j + 1 < q ? v.y : 0u) + (4 * j + 2 < q ? v.z : 0u) +
                         (4 * j + 3 < q ? v.w : 0u);
            }
            const uint32_t x0 = philox4x32_10_x0(c0, c1 + (uint32_t)ply, c2, c3, k0, k1);
            const unsigned t = (unsigned)(((uint64_t)(x0 >> 8) * S) >> 24);          // 24 x 31 bits: 64-bit product; t < S
            int mv = BKT_MOVE_NONE - 1;                              // not this thread's to write
            if (done || S == 0) { if (q == 0) mv = done ? BKT_MOVE_NONE : BK_PASS; }
            else if (mine && below <= t && t - below < w) mv = q;
            if (mv >= BKT_MOVE_NONE) {
                L.mv[p] = mv;
                if (hrow) hrow[ply] = (int16_t)mv;
            }
            if (!done) {                                             // every thread of the row knows whether it passes
                const bool pass = S == 0;
                done = pass && last_pass;                            // as play_body: the second pass in a row
                last_pass = pass;
                ++played;
            }
        }
    }
    if (!live) return;
    if (q == 0) {
        plies[b] = played;
        status[b] = st_or;
    }
    if (hrow)                                                        // the plies this workgroup did not run
        for (int i = ply + q; i < max_plies; i += NN) hrow[i] = (int16_t)BKT_MOVE_NONE;
}

}  // namespace

extern "C" int bkt_tactical_codes(const void* pos, int batch, int32_t* codes, void* stream) {
    if (!pos || !codes || batch < 1 || batch > BKT_MAX_BATCH) return BKT_ERR_ARG;
    // the ply body takes records it may play on; with BKT_MOVE_NONE for every row it only reads them
    hipLaunchKernelGGL(tactical_codes_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(const_cast<void*>(pos)), batch, codes);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

extern "C" int bkt_tactical_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                     const uint16_t* tactics, int max_plies, uint8_t* over, int32_t* plies, int16_t* moves,
                                     int32_t* status, void* stream) {
    if (!pos || !counters || !tactics || !over || !plies || !status || batch < 1 || batch > BKT_MAX_BATCH || max_plies < 1 ||
        max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(tactical_playouts_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(pos), batch, (uint32_t)seed, (uint32_t)(seed >> 32), counters, table,
                       tactics, max_plies, over, plies, moves, status);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

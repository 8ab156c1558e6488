// bk_playout_pat.hip -- the translation unit of the device Go rules in libbktrain.so: bk_playout_mc.hip as it is (textually,
// and through it bk_playout.hip, so that both still compile alone for the resource tests that pin their kernels), and
// appended after them the pattern-weighted playouts of bokego_amd/patterns.py (include/bokego_train.h):
// bkt_pattern_codes, the 3x3 pattern index of every point of a record, and bkt_pattern_playouts, bkt_random_playouts with a
// weighted draw.  bk_playout_tac.hip, included as text at the end, adds the tactical playouts on top of these.
//
// The index of a point s = 9r + c, relative to the side to move: the eight neighbours in the order (-1,0) (+1,0) (0,-1)
// (0,+1) (-1,-1) (-1,+1) (+1,-1) (+1,+1) give two bits each (0 empty, 1 the mover's stone, 2 the opponent's, 3 off the
// board), slot i at bit 2i; bit 16 is `near`: the record's last move is a board point at most one step away (itself
// included).  A table is uint16[131072]; the weight of a point is max(entry, 1).
//
// pattern_playouts_kernel is random_playouts_kernel with another step 2.  Per ply, after play_body<true> has left the
// playable set P in LDS: every thread reads its own board byte back (it wrote it itself), two ballots give the stone sets,
// a playable point looks its weight up and all of a row's weights go to LDS (0 outside P); after one barrier every thread
// sums the row's entries below its own point and the whole row, S <= 81 * 65535 < 2^23; t = ((x0 >> 8) * S) >> 24 in 64
// bits, and the move is the point whose interval [below, below + w) holds t -- exactly one, since t < S -- or BK_PASS when
// S == 0.  The side to move and the last move are carried in registers (the parity flips with every ply played; the move
// just played is still in L.mv), so nothing is read that another thread wrote to global memory.  All barriers and the exit
// test are workgroup-uniform; nothing crosses workgroups; no atomics, no spinning; integer work and plain vector stores.
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

__global__ void __launch_bounds__(256) pattern_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                               const uint32_t* __restrict__ counters,
                                                               const uint16_t* __restrict__ table, int max_plies,
                                                               unsigned char* over, int32_t* __restrict__ plies,
                                                               int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ PlyLds L;
    __shared__ PatLds W;
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
    int16_t* const hrow = hist ? hist + (size_t)b * max_plies : nullptr;   // per thread: two uniform values less in the loop
    int played = 0, st_or = 0, ply = 0;
    for (;; ++ply) {                                                 // round `ply` selects ply `ply`; the body before it
        __syncthreads();                                             // plays ply `ply - 1` (round 0: no move, the start sets)
        play_one_ply(pos, B, over, &L);
        if (live && q == 0) st_or |= L.st[p];
        if (ply == max_plies) break;
        if (!__syncthreads_or(live && !done)) break;                 // (the barrier also publishes L.playable)
        const bool mine = live && !done && L.playable[NN * pp + q] != 0;
        const int stone = live ? (signed char)pos[(size_t)b * BK_POS_BYTES + q] : 0;   // this thread's own store
        publish_ballots(W.bal, tid, stone == BK_BLACK, stone == BK_WHITE);
        const int just = L.mv[pp];                                   // the move the body has just played, if any
        if (just > BKT_MOVE_NONE) lm = just;
        __syncthreads();
        unsigned w = 0;
        if (mine) w = point_weight(&W, table, pp, q, lm, ((turn0 + played) & 1) != 0);
        if (p < PPW) W.w[p][q] = w;
        __syncthreads();
        if (live) {
            unsigned S = 0, below = 0;
            const uint4* row = reinterpret_cast<const uint4*>(W.w[pp]);
#pragma unroll 1                                                     // unrolled, the 84 loop-invariant compares fill the SGPRs
            for (int j = 0; j < PAT_ROW / 4; ++j) {
                const uint4 v = row[j];
                S += v.x + v.y + v.z + v.w;
                below += (4 * j < q ? v.x : 0u) + (4 * j + 1 < q ? v.y : 0u) + (4 * j + 2 < q ? v.z : 0u) +
                         (4 * j + 3 < q ? v.w : 0u);
            }
            const uint32_t x0 = philox4x32_10_x0(c0, c1 + (uint32_t)ply, c2, c3, k0, k1);
            const unsigned t = (unsigned)(((uint64_t)(x0 >> 8) * S) >> 24);          // 24 x 23 bits: 64-bit product
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

extern "C" int bkt_pattern_codes(const void* pos, int batch, int32_t* codes, void* stream) {
    if (!pos || !codes || batch < 1 || batch > BKT_MAX_BATCH) return BKT_ERR_ARG;
    hipLaunchKernelGGL(pattern_codes_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), batch, codes);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

extern "C" int bkt_pattern_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                    int max_plies, uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status,
                                    void* stream) {
    if (!pos || !counters || !table || !over || !plies || !status || batch < 1 || batch > BKT_MAX_BATCH || max_plies < 1 ||
        max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(pattern_playouts_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(pos), batch, (uint32_t)seed, (uint32_t)(seed >> 32), counters, table,
                       max_plies, over, plies, moves, status);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

#include "bk_playout_tac.hip"   // the tactical playouts: text, part of this translation unit

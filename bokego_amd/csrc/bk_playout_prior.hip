// bk_playout_prior.hip -- the move weights of a position in ONE launch: bkt_move_weights (include/bokego_train.h has the
// definition) gives every point the weight bkt_tactical_playouts' draw gives it at the first ply of a playout from the
// record as it stands, 0 off the playable set (bokego_amd/rollout.py move_weights, the pattern term of amaf_prior;
// DESIGN 22).  Before, that took bkt_pattern_codes, bkt_tactical_codes -- the whole ply body -- and bkt_playout_step plus
// gathers.  A translation unit of its own in libbktrain.so, beside bk_playout_owner.hip: bk_playout.hip and the
// text-include chain above it define the library's entry points and stay exactly as the resource tests pin them, so what
// this kernel needs of them -- meets, point, position_set, the pattern index (bk_playout_pat.hip), the tactical code
// (bk_playout_tac.hip) and the eye test and pending liberty refresh of play_body (bk_playout.hip, steps 7 and 4) -- is
// repeated here on purpose.  bk_encode_dev.h is a header: the planes are bk_enc::encode_points itself.
#include "bk_encode_dev.h"

#include "../../include/bokego_go.h"
#include "../../include/bokego_train.h"

namespace {

using namespace bk_enc;

constexpr int OFF_LIBS = 81, OFF_VALID = 162, OFF_KO = 164;

__device__ __forceinline__ BB point(int s) { return single(s / 27, 1u << (s % 27)); }
__device__ __forceinline__ bool meets(BB a, BB b) { return ((a.w[0] & b.w[0]) | (a.w[1] & b.w[1]) | (a.w[2] & b.w[2])) != 0; }
__device__ __forceinline__ BB position_set(const unsigned (&bal)[8], int p) {   // the 81 bits of seat p < PPW
    BB s;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
        const int off = NN * p + 27 * kk, i = off >> 5, sh = off & 31;           // off + 27 <= 243: i + 1 <= 7
        s.w[kk] = (unsigned)((((unsigned long long)bal[i + 1] << 32) | bal[i]) >> sh) & M27;
    }
    return s;
}

// bk_playout_pat.hip's index: two bits per neighbour relative to the mover, bit 16 `near`.
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

struct PriorLds {                         // 4016 bytes
    EncLds enc;                           // 3952: the stone ballots and the chains, encode_points' own
    unsigned nbr[2][8];                   // 64: the ballots of the 4 waves: the mover's stones in atari | the opponent's with two liberties
};

// Three records per workgroup, one thread per point (the encoder's seating; threads 243..255 and the seats of a tail
// workgroup beyond the batch load nothing and store nothing).
//   1. encode_points gives the thread the planes of its point that do not depend on the liberty cache -- legal (5), la
//      (13..19), cap (20..26) -- and leaves the stone ballots and every stone's chain mask in LDS.
//   2. Planes 6 and 7 are the cache AFTER the refresh bk_features_batch_u8(fresh = 0) does first (play_body step 4 for an
//      untouched record: every chain when the cache is invalid, else the chains at the last move and next to it when the
//      cached count there is 0): a stone's thread takes the exact count from its own chain mask, which it wrote itself.
//      What a neighbour needs of a point are two bits, plane 0 & plane 6 and plane 1 & plane 7: one ballot set, ONE barrier.
//   3. E and G are the neighbourhood of the point meeting those sets; the pattern index comes from the stone sets and the
//      last move, the eye from mask algebra on them; two table reads, one plain vector store.
// Integers only, no atomics, nothing shared between workgroups; the barriers (two inside encode_points, one here) are
// passed by every thread of the workgroup.
__global__ void __launch_bounds__(256) move_weights_kernel(const unsigned char* __restrict__ pos, int B,
                                                           const uint16_t* __restrict__ table,
                                                           const uint16_t* __restrict__ tactics,
                                                           uint32_t* __restrict__ weights) {
    __shared__ PriorLds S;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const unsigned char* rec0 = pos + (size_t)b0 * BK_POS_BYTES;
    unsigned char v[27];
    bool live;
    int p, q;
    encode_points(rec0, B - b0, tid, S.enc, v, live, p, q);
    const int pp = p < PPW ? p : 0;
    const int k = q / 27;
    const BB me_pt = single(k, 1u << (q - 27 * k));
    const BB black = position_set(S.enc.bal[0], pp), white = position_set(S.enc.bal[1], pp);

    int lm = BK_NO_MOVE;
    bool wtm = false, own1 = false, opp2 = false;
    if (live) {
        const unsigned char* rec = rec0 + p * BK_POS_BYTES;
        lm = (short)(*reinterpret_cast<const unsigned*>(rec + OFF_KO) >> 16);
        wtm = (v[3] == 0);                                           // plane 3: black to move
        if (v[2] == 0) {                                             // a stone: its cached liberty count, refreshed
            int libs = rec[OFF_LIBS + q];
            const uint4 ch = S.enc.chain[p][q];                      // this thread's own store
            const BB x{{ch.x, ch.y, ch.z}};
            bool exact = rec[OFF_VALID] == 0;
            if (!exact && lm >= 0 && lm < NN && rec[OFF_LIBS + lm] == 0) exact = meets(x, point(lm) | dilate(point(lm)));
            if (exact) libs = popc(dilate(x) & ~(black | white));
            own1 = v[0] != 0 && libs == 1;
            opp2 = v[1] != 0 && libs == 2;
        }
    }
    const unsigned long long b1 = __ballot(own1), b2 = __ballot(opp2);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        S.nbr[0][2 * w] = (unsigned)b1; S.nbr[0][2 * w + 1] = (unsigned)(b1 >> 32);
        S.nbr[1][2 * w] = (unsigned)b2; S.nbr[1][2 * w + 1] = (unsigned)(b2 >> 32);
    }
    __syncthreads();
    if (!live) return;

    unsigned w = 0;
    if (v[5]) {
        const BB mine = wtm ? white : black, theirs = wtm ? black : white;
        const BB around = dilate(me_pt);
        bool eye = !meets(around, ~mine);                            // every on-board neighbour is the mover's stone
        if (eye) {                                                   // bk_pos_possible_eye's diagonal count
            const int r = q / 9, c = q - 9 * r;
            int on_board = 0, faults = 0;
            if (r + 1 < 9 && c + 1 < 9) { on_board += 1; faults += (int)meets(theirs, point(q + 10)); }
            if (r + 1 < 9 && c >= 1) { on_board += 1; faults += (int)meets(theirs, point(q + 8)); }
            if (r >= 1 && c >= 1) { on_board += 2; faults += 2 * (int)meets(theirs, point(q - 10)); }   // listed twice
            if (on_board < 4) ++faults;
            eye = faults <= 1;
        }
        if (!eye) {
            unsigned P = 256u, T = 256u;
            if (table) {
                P = table[pattern_index(mine, theirs, q, lm)];
                P = P ? P : 1u;
            }
            if (tactics) {
                unsigned la = 0, cap = 0;                            // at most one of each seven is non-zero
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    la |= v[13 + i];
                    cap |= v[20 + i];
                }
                const unsigned e = meets(around, position_set(S.nbr[0], pp)), g = meets(around, position_set(S.nbr[1], pp));
                T = tactics[(cap < 3u ? cap : 3u) | (la <= 1u ? 0u : la == 2u ? 1u : 2u) << 2 | e << 4 | g << 5];
            }
            w = (P * T) >> 8;                                        // < 2^32 before the shift
            w = w ? w : 1u;
        }
    }
    weights[(size_t)(b0 + p) * NN + q] = w;
}

}  // namespace

extern "C" int bkt_move_weights(const void* pos, int batch, const uint16_t* table, const uint16_t* tactics, uint32_t* weights,
                                void* stream) {
    if (!pos || !weights || batch < 1 || batch > BKT_MAX_BATCH) return BKT_ERR_ARG;
    hipLaunchKernelGGL(move_weights_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), batch, table, tactics, weights);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

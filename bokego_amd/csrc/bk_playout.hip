// bk_playout.hip -- the Go rules on the device: bkt_play_moves (include/bokego_train.h) plays one move on each of a batch
// of 192-byte bk_pos records (include/bokego_go.h) in place and writes the 27 feature planes of the result, so that a
// lock-step policy playout (bokego_amd/genvals.py, bokego_amd/reinforce.py) needs no host work per ply; bkt_area_score
// scores the final records (area_score_kernel, at the end of the namespace).  bkt_playout_step is the same body (play_body
// with STEP = true) for playouts that run to the end of the game (bokego_amd/rollout.py): it also passes, keeps the `over`
// flag of a game that two passes have ended, and writes the points a playout may play (legal and not the mover's own eye).
//
// Contract: byte identity with the host rules.  After the call every record equals what bk_pos_play(p, m) followed by
// bk_pos_liberties(p, tmp) leaves (bk_go.cpp), reserved bytes included, and the planes equal bk_features_batch_u8 of it.
// That keeps the reference's liberty cache (refresh_libs): refreshed before the move, and again after it unless the cached
// count at the (new) last move is non-zero -- captured points keep stale counts, and a stone played on such a point skips
// the second refresh.
//
// Mapping: the encoder's (bk_encode_dev.h).  One 256-thread workgroup holds three positions, one thread per point; 81-point
// sets are three 27-bit words built from wave ballots, and each stone's thread grows its chain in registers.  Every chain
// that a rule looks at is then a mask:
//   captured  = opponent chains next to the move whose only liberty is the move (the board before any removal);
//   new chain = the move + own chains next to it, its liberties = (its empty neighbours - the move) + captured points;
//   refresh before the move: chains at the old last move and its neighbours take their exact count (all chains when the
//                  cache is invalid);
//   refresh after it: the new chain takes its count, a surviving opponent chain next to the move loses the move's point.
// Each thread writes its own board and libs byte; thread 0 of a position writes the header and status.  The planes come
// from bk_enc::encode_points on an LDS copy of the updated record whose libs are the refreshed ones bk_features_batch_u8
// would use (for an untouched record, the refresh pending on it; the record itself stays untouched).
// The hash needs no table: bk_go.cpp's Zobrist entry i is splitmix64's mix of (i + 2) * 0x9E3779B97F4A7C15.
// The step (STEP): a row whose `over` flag is set, or whose move is <= BKT_MOVE_NONE, is an untouched record.  A pass is
// bk_pos_play(p, BK_PASS) + bk_pos_liberties: the header changes (ko out of the hash, side to move, turn, last move), and
// the liberty cache is computed only when it was invalid -- last_move is BK_PASS by then, so a refresh that was pending on
// the old last move does NOT happen.  `playable` is bk_pos_is_legal && bk_pos_possible_eye != the mover, on the record as
// it stands after the call: legality is plane 5 of the encoder; the eye is mask algebra on the updated stone sets (every
// on-board neighbour the mover's, and the reference's diagonal count, bk_go.cpp bk_pos_possible_eye: (r+1,c+1), (r+1,c-1)
// and (r-1,c-1) TWICE, one fault more when any of them is off the board, an eye when at most one fault).
// Integer work only; plain vector stores.
#include "bk_encode_dev.h"

#include "../../include/bokego_go.h"
#include "../../include/bokego_train.h"

namespace {

using namespace bk_enc;

constexpr int OFF_LIBS = 81, OFF_VALID = 162, OFF_KO = 164, OFF_TURN = 172, OFF_HASH = 184;
constexpr int Z_KO = 162, Z_FLIP = 243;  // Zobrist entries: 81 * (colour - 1) + point, 162 + ko point, 243 side to move

__device__ __forceinline__ uint64_t zobrist(int i) {
    uint64_t z = (uint64_t)(i + 2) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ BB point(int s) { return single(s / 27, 1u << (s % 27)); }
__device__ __forceinline__ bool meets(BB a, BB b) { return ((a.w[0] & b.w[0]) | (a.w[1] & b.w[1]) | (a.w[2] & b.w[2])) != 0; }
__device__ __forceinline__ int colour_at(BB black, BB white, int s) {
    const BB m = point(s);
    return meets(black, m) ? BK_BLACK : meets(white, m) ? BK_WHITE : BK_EMPTY;
}
__device__ __forceinline__ int first_point(BB a) {
    return a.w[0] ? __ffs(a.w[0]) - 1 : a.w[1] ? 27 + __ffs(a.w[1]) - 1 : 54 + __ffs(a.w[2]) - 1;
}

template <bool STEP>
__device__ __forceinline__ void play_body(unsigned char* __restrict__ pos, const int32_t* __restrict__ moves, int B,
                                          unsigned char* __restrict__ over, int32_t* __restrict__ status,
                                          unsigned char* __restrict__ planes, unsigned char* __restrict__ playable) {
    __shared__ EncLds S;
    __shared__ __align__(16) unsigned char rec[PPW * BK_POS_BYTES];   // the updated records, as the encoder reads them
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    const int k = q / 27;
    const unsigned bit = 1u << (q - 27 * k);

    // ---- the record, as this point's thread needs it ----
    unsigned char* dst = pos + (size_t)(b0 + (live ? p : 0)) * BK_POS_BYTES;
    int me_board = 0, my_libs = 0, valid = 0, ko = BK_NO_KO, lm = BK_NO_MOVE, turn = 0, mv = -1, libs_lm = 0, libs_mv = 0;
    if (live) {
        me_board = (signed char)dst[q];
        my_libs = dst[OFF_LIBS + q];
        valid = dst[OFF_VALID];
        const unsigned kl = *reinterpret_cast<const unsigned*>(dst + OFF_KO);   // ko | last_move << 16
        ko = (short)(kl & 0xffffu);
        lm = (short)(kl >> 16);
        turn = *reinterpret_cast<const int*>(dst + OFF_TURN);
        mv = moves[b0 + p];
        if (STEP && over && over[b0 + p]) mv = BKT_MOVE_NONE;          // read before the first barrier, written after the last
        if (lm >= 0) libs_lm = dst[OFF_LIBS + lm];
        if (mv >= 0 && mv < NN) libs_mv = dst[OFF_LIBS + mv];
    }

    // ---- 1. bitboards from wave ballots (as bk_enc::encode_points) ----
    const unsigned long long bb = __ballot(me_board == BK_BLACK), bw = __ballot(me_board == BK_WHITE);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        S.bal[0][2 * w] = (unsigned)bb; S.bal[0][2 * w + 1] = (unsigned)(bb >> 32);
        S.bal[1][2 * w] = (unsigned)bw; S.bal[1][2 * w + 1] = (unsigned)(bw >> 32);
    }
    __syncthreads();
    BB black, white;
    {
        const int pp = p < PPW ? p : 0;
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            const int off = NN * pp + 27 * kk, i = off >> 5, sh = off & 31;
            const unsigned long long b2 = ((unsigned long long)S.bal[0][i + 1] << 32) | S.bal[0][i];
            const unsigned long long w2 = ((unsigned long long)S.bal[1][i + 1] << 32) | S.bal[1][i];
            black.w[kk] = (unsigned)(b2 >> sh) & M27;
            white.w[kk] = (unsigned)(w2 >> sh) & M27;
        }
    }
    const BB empty = ~(black | white);

    // ---- 2. this stone's chain and liberties, grown in registers; published with the chain's only liberty ----
    const bool stone = live && me_board != BK_EMPTY;
    BB x = single(k, bit), lib{{0, 0, 0}};
    {
        const BB own = me_board == BK_BLACK ? black : white;
        bool changed = stone;
        BB d = dilate(x);
        for (;;) {                         // wave-uniform exit
            const BB nx = (x | d) & own;
            changed = changed && (nx != x);
            if (!__any(changed)) break;
            if (changed) x = nx;
            d = dilate(x);
        }
        if (stone) {
            lib = d & empty;
            S.chain[p][q] = make_uint4(x.w[0], x.w[1], x.w[2], popc(lib) == 1 ? (unsigned)first_point(lib) : 255u);
        }
    }
    __syncthreads();

    // ---- 3. the move (every thread of a position computes the same outcome) ----
    const int me = (turn & 1) ? BK_WHITE : BK_BLACK, opp = BK_BLACK + BK_WHITE - me;
    int st = 0, new_ko = BK_NO_KO, la = 0, cap_dup = 0;
    BB cap{{0, 0, 0}}, newchain{{0, 0, 0}};
    if (live && mv >= 0) {
        if (mv >= NN) st = BK_ILLEGAL_OFF_BOARD;
        else if (mv == ko) st = BK_ILLEGAL_KO;
        else if (colour_at(black, white, mv) != BK_EMPTY) st = BK_ILLEGAL_NOT_EMPTY;
        else {
            const int r = mv / 9, c = mv - 9 * r;
            const int nbr[4] = {mv + 9, mv - 9, mv + 1, mv - 1};
            const bool nv[4] = {r + 1 < 9, r >= 1, c + 1 < 9, c >= 1};
            bool all_opp = true;            // possible_ko: every neighbour an opponent stone
            newchain = point(mv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!nv[j]) continue;
                const int bt = colour_at(black, white, nbr[j]);
                all_opp = all_opp && bt == opp;
                if (bt == BK_EMPTY) continue;
                const uint4 ch = S.chain[p][nbr[j]];
                const BB cx{{ch.x, ch.y, ch.z}};
                if (bt == opp) {
                    if (ch.w == (unsigned)mv) { cap = cap | cx; cap_dup += popc(cx); }
                } else {
                    newchain = newchain | cx;
                }
            }
            const BB d = dilate(newchain);
            la = popc((d & empty & ~point(mv)) | (cap & d));
            if (la == 0) st = BK_ILLEGAL_SUICIDE;
            else if (cap_dup == 1 && all_opp) new_ko = first_point(cap);
        }
    }
    const bool legal = live && mv >= 0 && st == 0;
    const bool passed = STEP && live && mv == BK_PASS;

    // ---- 4. the liberty cache: refresh_libs before the move (libs1), and after it (libs2) ----
    int libs1 = my_libs;
    if (!valid) libs1 = stone ? popc(lib) : 0;
    else if (lm >= 0 && libs_lm == 0 && stone && meets(x, point(lm) | dilate(point(lm)))) libs1 = popc(lib);
    const bool captured = meets(cap, single(k, bit));
    int board2 = me_board, libs2 = libs1;
    if (legal) {
        if (q == mv) board2 = me;
        else if (captured) board2 = BK_EMPTY;
        if ((valid ? libs_mv : 0) == 0) {   // the cached count at the new last move, after the first refresh
            if (meets(newchain, single(k, bit))) libs2 = la;
            else if (me_board == opp && !captured && meets(x, dilate(point(mv)))) libs2 = popc(lib & ~point(mv));
        }
    }

    // ---- 5. write back (a legal move only) ----
    if (legal) {
        dst[q] = (unsigned char)board2;
        dst[OFF_LIBS + q] = (unsigned char)libs2;
        if (q == 0) {
            uint64_t h = *reinterpret_cast<const uint64_t*>(dst + OFF_HASH) ^ zobrist(81 * (me - 1) + mv) ^ zobrist(Z_FLIP);
            if (ko >= 0) h ^= zobrist(Z_KO + ko);
            if (new_ko >= 0) h ^= zobrist(Z_KO + new_ko);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk)
                for (unsigned w = cap.w[kk]; w; w &= w - 1) h ^= zobrist(81 * (opp - 1) + 27 * kk + __ffs(w) - 1);
            dst[OFF_VALID] = 1;
            *reinterpret_cast<unsigned*>(dst + OFF_KO) = (unsigned)(unsigned short)new_ko | ((unsigned)mv << 16);
            *reinterpret_cast<int*>(dst + OFF_TURN) = turn + 1;
            *reinterpret_cast<uint64_t*>(dst + OFF_HASH) = h;
        }
    }
    const int libs_pass = valid ? my_libs : (stone ? popc(lib) : 0);   // a pass: the cache only when it was invalid
    if (passed) {
        if (!valid) dst[OFF_LIBS + q] = (unsigned char)libs_pass;
        if (q == 0) {
            uint64_t h = *reinterpret_cast<const uint64_t*>(dst + OFF_HASH) ^ zobrist(Z_FLIP);
            if (ko >= 0) h ^= zobrist(Z_KO + ko);
            dst[OFF_VALID] = 1;
            *reinterpret_cast<unsigned*>(dst + OFF_KO) = (unsigned)(unsigned short)BK_NO_KO | ((unsigned)BK_PASS << 16);
            *reinterpret_cast<int*>(dst + OFF_TURN) = turn + 1;
            *reinterpret_cast<uint64_t*>(dst + OFF_HASH) = h;
            if (over && lm == BK_PASS) over[b0 + p] = 1;               // the second pass in a row ends the game
        }
    }
    if (live && q == 0) status[b0 + p] = st;
    if (!planes && !(STEP && playable)) return;                        // uniform: kernel arguments

    // ---- 6. the planes of the record as it now stands, libs refreshed as bk_features_batch_u8 refreshes them (an
    //         untouched record: libs1, the refresh pending on it; after a legal move libs2 is already refreshed) ----
    if (live) {
        unsigned char* r = rec + p * BK_POS_BYTES;
        r[q] = (unsigned char)board2;
        r[OFF_LIBS + q] = (unsigned char)(legal ? libs2 : passed ? libs_pass : libs1);
        if (q == 0) {
            *reinterpret_cast<unsigned*>(r + OFF_KO) =
                legal ? ((unsigned)(unsigned short)new_ko | ((unsigned)mv << 16))
                : passed ? ((unsigned)(unsigned short)BK_NO_KO | ((unsigned)BK_PASS << 16))
                         : ((unsigned)(unsigned short)ko | ((unsigned)lm << 16));
            *reinterpret_cast<int*>(r + OFF_TURN) = legal || passed ? turn + 1 : turn;
        }
    }
    __syncthreads();
    unsigned char v[27];
    bool enc_live;
    int ep, eq;
    encode_points(rec, B - b0, tid, S, v, enc_live, ep, eq);
    if (enc_live && planes) {
        unsigned char* out = planes + (size_t)(b0 + ep) * 2187 + eq;
#pragma unroll
        for (int i = 0; i < 27; ++i) out[i * NN] = v[i];
    }
    if (!STEP || !playable || !live) return;

    // ---- 7. the playable set of the record as it now stands: legal (plane 5) and not the mover's own one-point eye ----
    BB mine = me == BK_BLACK ? black : white, theirs = me == BK_BLACK ? white : black;
    if (legal) { mine = mine | point(mv); theirs = theirs & ~cap; }
    const bool flipped = legal || passed;                              // the side to move is now the other one
    const BB mover = flipped ? theirs : mine, other = flipped ? mine : theirs;
    bool eye = !meets(dilate(single(k, bit)), ~mover);                 // every on-board neighbour is the mover's stone
    if (eye) {
        const int r = q / 9, c = q - 9 * r;
        int on_board = 0, faults = 0;
        if (r + 1 < 9 && c + 1 < 9) { on_board += 1; faults += (int)meets(other, point(q + 10)); }
        if (r + 1 < 9 && c >= 1) { on_board += 1; faults += (int)meets(other, point(q + 8)); }
        if (r >= 1 && c >= 1) { on_board += 2; faults += 2 * (int)meets(other, point(q - 10)); }   // the table lists it twice
        if (on_board < 4) ++faults;
        eye = faults <= 1;
    }
    playable[(size_t)(b0 + p) * NN + q] = (unsigned char)(v[5] && !eye);
}

__global__ void __launch_bounds__(256) play_moves_kernel(unsigned char* __restrict__ pos, const int32_t* __restrict__ moves,
                                                         int B, int32_t* __restrict__ status,
                                                         unsigned char* __restrict__ planes) {
    play_body<false>(pos, moves, B, nullptr, status, planes, nullptr);
}

__global__ void __launch_bounds__(256) playout_step_kernel(unsigned char* __restrict__ pos, const int32_t* __restrict__ moves,
                                                           int B, unsigned char* __restrict__ over,
                                                           int32_t* __restrict__ status, unsigned char* __restrict__ planes,
                                                           unsigned char* __restrict__ playable) {
    play_body<true>(pos, moves, B, over, status, planes, playable);
}

// The area score (bk_pos_area_score): an empty point's thread grows its region through the empty points as a stone's thread
// grows its chain; the region is a colour's if its neighbour set meets that colour and not the other.  The two area sets go
// through a second round of ballots and thread 0 of a position adds the popcounts.  The records are only read.
__device__ __forceinline__ void publish_ballots(unsigned (&bal)[2][8], int tid, bool a, bool b) {
    const unsigned long long ba = __ballot(a), bb = __ballot(b);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        bal[0][2 * w] = (unsigned)ba; bal[0][2 * w + 1] = (unsigned)(ba >> 32);
        bal[1][2 * w] = (unsigned)bb; bal[1][2 * w + 1] = (unsigned)(bb >> 32);
    }
}
__device__ __forceinline__ BB position_set(const unsigned (&bal)[8], int p) {   // the 81 bits of position p < PPW
    BB s;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
        const int off = NN * p + 27 * kk, i = off >> 5, sh = off & 31;           // off + 27 <= 243: i + 1 <= 7
        s.w[kk] = (unsigned)((((unsigned long long)bal[i + 1] << 32) | bal[i]) >> sh) & M27;
    }
    return s;
}

__global__ void __launch_bounds__(256) area_score_kernel(const unsigned char* __restrict__ pos, int B, float komi,
                                                         float* __restrict__ score, signed char* __restrict__ owner) {
    __shared__ unsigned stones[2][8], area[2][8];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    const int k = q / 27;
    const int me_board = live ? (signed char)pos[(size_t)(b0 + p) * BK_POS_BYTES + q] : 0;

    publish_ballots(stones, tid, me_board == BK_BLACK, me_board == BK_WHITE);
    __syncthreads();
    const int pp = p < PPW ? p : 0;
    const BB black = position_set(stones[0], pp), white = position_set(stones[1], pp);
    const BB empty = ~(black | white);

    BB x = single(k, 1u << (q - 27 * k));
    bool changed = live && me_board == BK_EMPTY;
    BB d = dilate(x);
    for (;;) {                             // wave-uniform exit
        const BB nx = (x | d) & empty;
        changed = changed && (nx != x);
        if (!__any(changed)) break;
        if (changed) x = nx;
        d = dilate(x);
    }
    int own = me_board == BK_BLACK ? 1 : me_board == BK_WHITE ? -1 : 0;
    if (live && me_board == BK_EMPTY) own = (int)meets(d, black) - (int)meets(d, white);

    publish_ballots(area, tid, live && own > 0, live && own < 0);
    if (live && owner) owner[(size_t)(b0 + p) * NN + q] = (signed char)own;
    __syncthreads();
    if (live && q == 0) score[b0 + p] = (float)popc(position_set(area[0], p)) - ((float)popc(position_set(area[1], p)) + komi);
}

}  // namespace

extern "C" int bkt_play_moves(void* pos, const int32_t* moves, int batch, int32_t* status, uint8_t* planes, void* stream) {
    if (!pos || !moves || !status || batch < 1 || batch > BKT_MAX_BATCH) return BKT_ERR_ARG;
    hipLaunchKernelGGL(play_moves_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(pos), moves, batch, status, planes);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

extern "C" int bkt_playout_step(void* pos, const int32_t* moves, int batch, uint8_t* over, int32_t* status, uint8_t* planes,
                                uint8_t* playable, void* stream) {
    if (!pos || !moves || !status || batch < 1 || batch > BKT_MAX_BATCH) return BKT_ERR_ARG;
    hipLaunchKernelGGL(playout_step_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(pos), moves, batch, over, status, planes, playable);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

extern "C" int bkt_area_score(const void* pos, int batch, float komi, float* score, int8_t* owner, void* stream) {
    if (!pos || !score || batch < 1 || batch > BKT_MAX_BATCH || !(komi - komi == 0.0f)) return BKT_ERR_ARG;   // komi finite
    hipLaunchKernelGGL(area_score_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), batch, komi, score, reinterpret_cast<signed char*>(owner));
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

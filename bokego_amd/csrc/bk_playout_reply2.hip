// bk_playout_reply2.hip -- included as text at the end of bk_playout_pat.hip, after bk_playout_reply.hip (it is no
// translation unit of its own): last-good-reply playouts keyed by the last TWO moves (LGRF-2; include/bokego_train.h has the
// table and the two rules).  bkt_reply2_playouts is bkt_reply_playouts whose draw asks the pair entry first and
// the single entry (plane 81) second; bkt_reply2_update is the sequential fold of DESIGN 24 over 13,284 entries, computed
// event-parallel: its cost is O(events) and its scratch a constant, whatever the number of records.

namespace {

constexpr int REPLY2_PLANE = NN * NN;                                // one plane [p2][...]: 81 entries per p2
constexpr int REPLY2_COLOUR = (NN + 1) * NN;                         // replies2[c]: 82 planes
constexpr int REPLY2_ENTRIES = 2 * REPLY2_COLOUR;                    // 13,284
constexpr int REPLY2_DWORDS = REPLY2_ENTRIES / 4;                    // 3,321: the table is a whole number of dwords
constexpr int REPLY2_NO_MOVE = -100;                                 // lm2 before any ply: equals no point, no pass
static_assert(REPLY2_ENTRIES % 4 == 0, "the table is staged by dwords");

// The fifth draw: ReplyDraw's form (bk_playout_reply.hip) with one table of 13,284 bytes for all rows, staged in LDS by
// dword loads (13 per thread) and published by the ply loop's first barrier.  lm2 is the move two plies back: the inner
// draw's `lm` as it stood before inner.publish() took the move just played, kept whenever there was one (L.mv is read
// before publish()'s barrier, as the inner draws read it).  At ply 0 there is none; at ply 1 it is the record's last move.
// Behind the inner draw's last barrier the thread reads two LDS bytes, the same addresses in a whole row: the pair entry
// [c][lm2][lm] when lm and lm2 are board points (else the single entry again), and the single entry [c][81][lm] (lm = 0
// when it is no board point; the result is then not used).  Each is compared (<= 80) before it indexes L.playable.  The
// lookups are selects, not branches: nested branches cost the tactical kernel two SGPR spills.  No barrier is reached.
template <class Inner>
struct Reply2Draw {
    Inner inner;
    const uint32_t* __restrict__ replies2;                           // 4-byte aligned: checked by the entry point
    int q, reply, lm2;
    static __device__ __forceinline__ uint32_t* lds() {
        __shared__ uint32_t table[REPLY2_DWORDS];
        return table;
    }
    __device__ __forceinline__ void start(Seat s, int last_move, int turn) {
#pragma unroll 1
        for (int i = s.tid; i < REPLY2_DWORDS; i += 256) lds()[i] = replies2[i];
        q = s.q, lm2 = REPLY2_NO_MOVE;
        inner.start(s, last_move, turn);
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds& L, bool mine, int played) {
        if (L.mv[s.pp] > BKT_MOVE_NONE) lm2 = inner.lm;              // a move was just played: the one before it moves on
        inner.publish(s, L, mine, played);
        const int lm = inner.lm;
        const bool asks = lm >= 0 && lm < NN, pair = asks && lm2 >= 0 && lm2 < NN;   // selects, not branches: two LDS reads
        const uint8_t* t = reinterpret_cast<const uint8_t*>(lds()) + (((inner.turn0 + played) & 1) ? REPLY2_COLOUR : 0) + (asks ? lm : 0);
        const uint8_t* own = L.playable + NN * s.pp;
        const int r1 = t[REPLY2_PLANE], r2 = t[pair ? NN * lm2 : REPLY2_PLANE];
        const bool ok1 = asks && r1 < NN && own[r1 < NN ? r1 : 0] != 0, ok2 = pair && r2 < NN && own[r2 < NN ? r2 : 0] != 0;
        reply = ok2 ? r2 : ok1 ? r1 : -1;
    }
    __device__ __forceinline__ unsigned total(Seat s) { return inner.total(s); }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned S) const {
        return reply >= 0 ? q == reply : inner.picks(r24, S);
    }
};

__global__ void __launch_bounds__(256) lgr2_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                            const uint32_t* __restrict__ counters,
                                                            const uint16_t* __restrict__ table,
                                                            const uint16_t* __restrict__ tactics,
                                                            const uint32_t* __restrict__ replies2, int max_plies,
                                                            unsigned char* over, int32_t* __restrict__ plies,
                                                            int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             Reply2Draw<WeightedDraw<OptionalTacticalWeight>>{{{table, tactics}}, replies2});
}

__global__ void __launch_bounds__(256) lgr2_uniform_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                    const uint32_t* __restrict__ counters,
                                                                    const uint32_t* __restrict__ replies2, int max_plies,
                                                                    unsigned char* over, int32_t* __restrict__ plies,
                                                                    int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ unsigned sel[8];
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             Reply2Draw<TrackedUniformDraw>{{UniformDraw{sel}, 0, 0}, replies2});
}

// ---- the update ---------------------------------------------------------------------------------------------------------
// The fold has a closed form per entry.  An event of order o = row * max_plies + ply (the fold's own order) carries a move m
// and is a store (the mover won the row) or a clear.  With K the largest (o + 1) << 8 | m over the entry's stores -- its
// last store and the value v it left -- the entry ends as 255 if a clear of order > o carries m == v, else as v; with no
// store (K == 0) it ends as 255 if any clear carries m equal to the value on entry, else unchanged.  Scratch: a uint64 key
// per entry, then a flag byte per entry.  Four launches in stream order; within one, integer max is order-independent and
// a flag is only ever written with the value 1, so the result does not depend on the scheduling.

constexpr int REPLY2_WAVES = 4;                                      // rows per workgroup of the two event passes
constexpr size_t REPLY2_FLAGS_AT = (size_t)REPLY2_ENTRIES * sizeof(unsigned long long);
constexpr size_t REPLY2_SCRATCH = REPLY2_FLAGS_AT + REPLY2_ENTRIES;  // 119,556 bytes; keys and flags both whole dwords

__global__ void __launch_bounds__(256) lgr2_init_kernel(uint32_t* __restrict__ scratch) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < REPLY2_SCRATCH / 4) scratch[i] = 0u;
}

// The seating of both event passes: a wave per row, lanes over plies in chunks of 64.  Lane j of chunk k0 looks at ply
// t = k0 + j: m = moves[t], p1 the move before (the record's last move at t = 0), p2 the one before that (the record's
// last move at t = 1, none at t = 0).  The row ends at the first m <= BKT_MOVE_NONE: the lowest set bit of a ballot,
// carried across chunks by leaving the loop -- wave-uniform, as the loop bound is.  on_event(entry, order, m, mover_won)
// is called for the single entry [c][81][p1] and, when p2 is a board point, for the pair entry [c][p2][p1]; m, p1 and p2
// are compared (0..80) before they index, so entry < REPLY2_ENTRIES.
template <class OnEvent>
__device__ __forceinline__ void lgr2_events(const unsigned char* __restrict__ pos, const int16_t* __restrict__ moves,
                                            int max_plies, const uint8_t* __restrict__ won, long long rows, int playouts,
                                            OnEvent on_event) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * REPLY2_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                                         // wave-uniform; no barrier below
    const unsigned char* rec = pos + (size_t)(row / playouts) * BK_POS_BYTES;
    const int lm0 = (short)(*reinterpret_cast<const unsigned*>(rec + OFF_KO) >> 16);
    const int c0 = *reinterpret_cast<const int*>(rec + OFF_TURN) & 1;
    const bool win = won[row] != 0;
    const int16_t* src = moves + (size_t)row * max_plies;
    for (int k0 = 0; k0 < max_plies; k0 += 64) {
        const int t = k0 + lane;
        const bool in = t < max_plies;
        const int m = in ? (int)src[t] : BKT_MOVE_NONE;
        const unsigned long long ends = __ballot(m <= BKT_MOVE_NONE);
        const int first = ends ? __ffsll((long long)ends) - 1 : 64;  // the lanes below it are the row's plies
        if (lane < first && m >= 0 && m < NN) {
            const int p1 = t == 0 ? lm0 : (int)src[t - 1];
            if (p1 >= 0 && p1 < NN) {
                const int p2 = t == 0 ? REPLY2_NO_MOVE : t == 1 ? lm0 : (int)src[t - 2];
                const int c = c0 ^ (t & 1);
                const bool mover_won = win == ((t & 1) == 0);
                const unsigned long long order = (unsigned long long)row * (unsigned)max_plies + (unsigned)t;
                const int single = c * REPLY2_COLOUR + REPLY2_PLANE + p1;
                on_event(single, order, m, mover_won);
                if (p2 >= 0 && p2 < NN) on_event(single - REPLY2_PLANE + NN * p2, order, m, mover_won);
            }
        }
        if (ends) break;
    }
}

__global__ void __launch_bounds__(64 * REPLY2_WAVES) lgr2_store_kernel(const unsigned char* __restrict__ pos,
                                                                       const int16_t* __restrict__ moves, int max_plies,
                                                                       const uint8_t* __restrict__ won, long long rows,
                                                                       int playouts, unsigned long long* __restrict__ keys) {
    lgr2_events(pos, moves, max_plies, won, rows, playouts, [=](int entry, unsigned long long order, int m, bool mover_won) {
        if (mover_won) atomicMax(keys + entry, (order + 1) << 8 | (unsigned long long)m);
    });
}

__global__ void __launch_bounds__(64 * REPLY2_WAVES) lgr2_clear_kernel(const unsigned char* __restrict__ pos,
                                                                       const int16_t* __restrict__ moves, int max_plies,
                                                                       const uint8_t* __restrict__ won, long long rows,
                                                                       int playouts, const unsigned long long* __restrict__ keys,
                                                                       const uint8_t* __restrict__ replies2,
                                                                       uint8_t* __restrict__ flags) {
    lgr2_events(pos, moves, max_plies, won, rows, playouts, [=](int entry, unsigned long long order, int m, bool mover_won) {
        if (mover_won) return;
        const unsigned long long key = keys[entry];
        const bool clears = key == 0 ? (int)replies2[entry] == m : order + 1 > key >> 8 && (int)(key & 255u) == m;
        if (clears) flags[entry] = 1;
    });
}

__global__ void __launch_bounds__(256) lgr2_finish_kernel(const unsigned long long* __restrict__ keys,
                                                          const uint8_t* __restrict__ flags, uint8_t* __restrict__ replies2) {
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= REPLY2_ENTRIES) return;
    const unsigned long long key = keys[e];
    if (flags[e]) replies2[e] = (uint8_t)BKT_REPLY_NONE;
    else if (key) replies2[e] = (uint8_t)(key & 255u);
}

inline bool reply2_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int bkt_reply2_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                   const uint16_t* tactics, const uint8_t* replies2, int max_plies, uint8_t* over,
                                   int32_t* plies, int16_t* moves, int32_t* status, void* stream) {
    if (!replies2 || !reply2_aligned(replies2)) return BKT_ERR_ARG;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(replies2);
    if (!table && !tactics)
        return launch_playouts(lgr2_uniform_playouts_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status,
                               stream, words);
    return launch_playouts(lgr2_playouts_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream,
                           table, tactics, words);
}

extern "C" size_t bkt_reply2_scratch_bytes(void) { return REPLY2_SCRATCH; }

extern "C" int bkt_reply2_update(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records,
                                 int playouts, uint8_t* replies2, void* scratch, void* stream) {
    if (!pos || !moves || !won || !replies2 || !scratch || !reply2_aligned(replies2) || (reinterpret_cast<uintptr_t>(scratch) & 7u) ||
        records < 1 || playouts < 1 || (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 ||
        max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    const long long rows = (long long)records * playouts;
    const dim3 seats((unsigned)((rows + REPLY2_WAVES - 1) / REPLY2_WAVES)), entries((REPLY2_ENTRIES + 255) / 256);
    unsigned long long* keys = static_cast<unsigned long long*>(scratch);
    uint8_t* flags = static_cast<uint8_t*>(scratch) + REPLY2_FLAGS_AT;
    const unsigned char* p = static_cast<const unsigned char*>(pos);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lgr2_init_kernel, dim3((unsigned)((REPLY2_SCRATCH / 4 + 255) / 256)), dim3(256), 0, s,
                       static_cast<uint32_t*>(scratch));
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(lgr2_store_kernel, seats, dim3(64 * REPLY2_WAVES), 0, s, p, moves, max_plies, won, rows, playouts, keys);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(lgr2_clear_kernel, seats, dim3(64 * REPLY2_WAVES), 0, s, p, moves, max_plies, won, rows, playouts, keys,
                       static_cast<const uint8_t*>(replies2), flags);
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    hipLaunchKernelGGL(lgr2_finish_kernel, entries, dim3(256), 0, s, keys, flags, replies2);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

#include "bk_playout_nast.hip" // move values keyed by the previous move (NAST): text, behind the entry points above

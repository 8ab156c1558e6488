// bk_playout_mc.hip -- the translation unit of the device Go rules in libbktrain.so: bk_playout.hip as it is (textually, so
// that its kernels and play_body stay untouched and bk_playout.hip still compiles alone, three kernels, for the resource
// tests that pin it), and appended after it what whole playouts in ONE launch need, for the Monte-Carlo value of
// bokego_amd/rollout.py: the ply loop that every playout kernel of the library runs (playouts<Draw>), the host
// launch they share (launch_playouts), and the uniform draw with its entry point bkt_random_playouts
// (include/bokego_train.h).  The weighted draws are bk_playout_pat.hip's and bk_playout_tac.hip's.
#include "bk_playout.hip"

namespace {

// Random123's philox4x32 with 10 rounds; bk_train.hip's sampler and reinforce.philox4x32_10 are the same function.
__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c2 = hi0 ^ c3 ^ k1;
        c1 = lo1;
        c3 = lo0;
    }
    return c0;
}

// What play_body reads and writes per row, in LDS: the move to play, its status, and the playable set it leaves behind.
struct PlyLds {
    int32_t mv[PPW], st[PPW];
    unsigned char playable[PPW * NN];
};

// One ply of the workgroup's rows.  play_body indexes its per-row arguments with b0 + p: shifted by -b0 they are the
// workgroup's own slots.  One call site, not inlined: inlined into the ply loop, the body's loop-invariant values are
// hoisted out of it and the kernel needs twice the registers of playout_step_kernel.
__device__ __noinline__ void play_one_ply(unsigned char* pos, int B, unsigned char* over, PlyLds* L) {
    const int b0 = blockIdx.x * PPW;
    play_body<true>(pos, L->mv - b0, B, over, L->st - b0, nullptr, L->playable - (size_t)b0 * NN);
}

// A thread's place: playout_step_kernel's mapping, three records per 256-thread workgroup, one thread per point.  Thread
// tid is point q of row p (pp: p, or 0 past the third row) of record rec, which it reads only if live: the row exists.
struct Seat {
    int tid, p, q, pp;
    bool live;
    const unsigned char* rec;
};

// Whole playouts of the workgroup's rows: every *_playouts_kernel is this function with its draw.  A ply is what the
// lock-step loop of rollout.finish_games does in three launches:
//   1. the playable set P of the record as it stands is the one play_body<true> left behind (LDS instead of global memory);
//   2. Philox4x32-10 with key (k0, k1) and the row's counter (c0, c1 + ply, c2, c3) gives x0, and the draw picks one point
//      of P with the 24 bits x0 >> 8, or the row passes (BK_PASS) when the draw's total over P is 0: no float, no fallback;
//   3. play_body<true> plays it on the record in global memory exactly as bkt_playout_step does (its `moves`, `status` and
//      `playable` arguments point into LDS, shifted so that the body's own row index b0 + p lands on slot p) and writes
//      the next playable set.
// The rows of a workgroup run in lock-step: a row that two passes have ended idles (BKT_MOVE_NONE: an untouched record)
// until all three are over or the cap is reached.  That exit test and every barrier, the draw's included, are
// workgroup-uniform; nothing is shared between workgroups; no atomics, no spinning; integer work and plain vector stores.
// `over` and the record header are written by a row's first thread and read by all of them one ply later: the barriers in
// between order them (workgroup scope is enough -- one workgroup owns a row for the whole launch).
//
// A Draw is one thread's share of step 2: start(seat, lm, turn) once, with the record's last move and turn on entry;
// play(), play_one_ply or a sibling that keeps more of what play_body computes; then per ply publish(seat, L, mine, played)
// by every thread of the workgroup -- what a row's threads need of each other goes to LDS, and a barrier ends it (mine: the
// thread's point is in P; played: the plies its row has played) -- and by live threads total(seat), the total over P that
// the 24 bits are scaled by, and picks(r24, total): whether the draw falls on this thread's point, true for one point of P.
// Its functions are inlined by force and take the seat by value, and its LDS is a static of its own, not a pointer it is
// handed: what reaches the __noinline__ helpers below them -- pp < 3, q < 81, LDS addresses -- then reaches them as the
// ranges and constants it is, as when the call stood in the kernel itself (24-bit multiplies, no 64-bit addresses).
template <class Draw>
__device__ __forceinline__ void playouts(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                         const uint32_t* __restrict__ counters, int max_plies, unsigned char* over,
                                         int32_t* __restrict__ plies, int16_t* __restrict__ hist,
                                         int32_t* __restrict__ status, Draw draw) {
    __shared__ PlyLds L;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    const int pp = p < PPW ? p : 0;
    const int b = b0 + (live ? p : 0);
    const Seat seat{tid, p, q, pp, live, pos + (size_t)b * BK_POS_BYTES};
    bool done = true, last_pass = false;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    int lm = BK_NO_MOVE, turn0 = 0;
    if (live) {
        done = over[b] != 0;
        lm = (short)(*reinterpret_cast<const unsigned*>(seat.rec + OFF_KO) >> 16);
        turn0 = *reinterpret_cast<const int*>(seat.rec + OFF_TURN);
        last_pass = lm == BK_PASS;
        c0 = counters[4 * (size_t)b], c1 = counters[4 * (size_t)b + 1];
        c2 = counters[4 * (size_t)b + 2], c3 = counters[4 * (size_t)b + 3];
        if (q == 0) L.mv[p] = BKT_MOVE_NONE;
    }
    draw.start(seat, lm, turn0);
    int16_t* const hrow = hist ? hist + (size_t)b * max_plies : nullptr;   // per thread: two uniform values less in the loop
    int played = 0, st_or = 0, ply = 0;
    for (;; ++ply) {                                                 // round `ply` selects ply `ply`; the body before it
        __syncthreads();                                             // plays ply `ply - 1` (round 0: no move, the start sets)
        draw.play(pos, B, over, &L);
        if (live && q == 0) st_or |= L.st[p];
        if (ply == max_plies) break;
        if (!__syncthreads_or(live && !done)) break;                 // (the barrier also publishes what the body wrote to LDS)
        const bool mine = live && !done && L.playable[NN * pp + q] != 0;
        draw.publish(seat, L, mine, played);
        if (live) {
            const unsigned total = draw.total(seat);
            int mv = BKT_MOVE_NONE - 1;                              // not this thread's to write
            if (done || total == 0) { if (q == 0) mv = done ? BKT_MOVE_NONE : BK_PASS; }
            else if (draw.picks(philox4x32_10_x0(c0, c1 + (uint32_t)ply, c2, c3, k0, k1) >> 8, total) && mine) mv = q;
            if (mv >= BKT_MOVE_NONE) {
                L.mv[p] = mv;
                if (hrow) hrow[ply] = (int16_t)mv;
            }
            if (!done) {                                             // every thread of the row knows whether it passes
                const bool pass = total == 0;
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

// The uniform draw: two ballots turn P into an 81-bit set, n = |P|, every point knows its rank in ascending point order,
// and the move is the point of rank (r24 * n) >> 24 (rollout.select_index).
struct UniformDraw {
    unsigned (&sel)[8];                                              // LDS: the playable points of the 4 waves, one bit each
    int k;
    unsigned below, rank;
    __device__ __forceinline__ void start(Seat s, int, int) {
        k = s.q / 27;
        below = (1u << (s.q - 27 * k)) - 1u;                         // this word's points before q
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        play_one_ply(pos, B, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds&, bool mine, int) const {
        const unsigned long long bal = __ballot(mine);
        if ((s.tid & 63) == 0) {
            sel[2 * (s.tid >> 6)] = (unsigned)bal;
            sel[2 * (s.tid >> 6) + 1] = (unsigned)(bal >> 32);
        }
        __syncthreads();
    }
    __device__ __forceinline__ unsigned total(Seat s) {
        const BB P = position_set(sel, s.pp);
        rank = (k > 0 ? __popc(P.w[0]) : 0) + (k > 1 ? __popc(P.w[1]) : 0) + __popc(word_of(P, k) & below);
        return (unsigned)popc(P);
    }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned n) const {
        return rank == (r24 * n) >> 24;                              // 24 x 7 bits, exact in 32
    }
};

__global__ void __launch_bounds__(256) random_playouts_kernel(unsigned char* __restrict__ pos, int B, uint32_t k0, uint32_t k1,
                                                              const uint32_t* __restrict__ counters, int max_plies,
                                                              unsigned char* over, int32_t* __restrict__ plies,
                                                              int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ unsigned sel[8];
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status, UniformDraw{sel});
}

// The argument check and the launch of the bkt_*_playouts entry points; `extra`: the kernel's own arguments, after counters.
template <class Kernel, class... Extra>
int launch_playouts(Kernel kernel, void* pos, int batch, uint64_t seed, const uint32_t* counters, int max_plies,
                    uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status, void* stream, Extra... extra) {
    if (!pos || !counters || !over || !plies || !status || batch < 1 || batch > BKT_MAX_BATCH || max_plies < 1 ||
        max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(pos), batch, (uint32_t)seed, (uint32_t)(seed >> 32), counters, extra...,
                       max_plies, over, plies, moves, status);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

}  // namespace

extern "C" int bkt_random_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, int max_plies, uint8_t* over,
                                   int32_t* plies, int16_t* moves, int32_t* status, void* stream) {
    return launch_playouts(random_playouts_kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream);
}

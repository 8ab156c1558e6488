// bk_playout_mc.hip -- the translation unit of the device Go rules in libbktrain.so: bk_playout.hip as it is (textually, so
// that its kernels and play_body stay untouched and bk_playout.hip still compiles alone, three kernels, for the resource
// tests that pin it), and appended after it bkt_random_playouts (include/bokego_train.h): whole uniformly random playouts
// in ONE launch, for the Monte-Carlo value of bokego_amd/rollout.py.
//
// random_playouts_kernel keeps playout_step_kernel's mapping -- three records per 256-thread workgroup, one thread per
// point -- and runs the ply loop itself.  A ply is what the lock-step loop of rollout.finish_games does in three launches:
//   1. the playable set P of the record as it stands is the one play_body<true> left behind (LDS instead of global memory);
//      two ballots turn it into an 81-bit set, n = |P|, and every point knows its rank in ascending point order;
//   2. Philox4x32-10 with key `seed` and the row's counter (c0, c1 + k, c2, c3) gives x0; the move is the point of rank
//      ((x0 >> 8) * n) >> 24 -- 24 x 7 bits, exact in 32 -- or BK_PASS when n == 0: no float, no fallback rule;
//   3. play_body<true> plays it on the record in global memory exactly as bkt_playout_step does (its `moves`, `status` and
//      `playable` arguments point into LDS, shifted so that the body's own row index b0 + p lands on slot p) and writes
//      the next playable set.
// The rows of a workgroup run in lock-step: a row that two passes have ended idles (BKT_MOVE_NONE: an untouched record)
// until all three are over or the cap is reached.  That exit test (__syncthreads_or) and every barrier are
// workgroup-uniform; nothing is shared between workgroups; no atomics, no spinning; integer work and plain vector stores.
// `over` and the record header are written by a row's first thread and read by all of them one ply later: the barriers in
// between order them (workgroup scope is enough -- one workgroup owns a row for the whole launch).
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

__global__ void __launch_bounds__(256) random_playouts_kernel(unsigned char* __restrict__ pos, int B, uint32_t k0, uint32_t k1,
                                                              const uint32_t* __restrict__ counters, int max_plies,
                                                              unsigned char* over, int32_t* __restrict__ plies,
                                                              int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ PlyLds L;
    __shared__ unsigned sel[8];                                      // the playable points of the 4 waves, one bit each
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * PPW;
    const int p = tid / NN, q = tid - NN * p;
    const bool live = p < PPW && b0 + p < B;
    const int pp = p < PPW ? p : 0;
    const int b = b0 + (live ? p : 0);
    const int k = q / 27;
    const unsigned below = (1u << (q - 27 * k)) - 1u;                // this word's points before q
    bool done = true, last_pass = false;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (live) {
        done = over[b] != 0;
        last_pass = (short)(*reinterpret_cast<const unsigned*>(pos + (size_t)b * BK_POS_BYTES + OFF_KO) >> 16) == BK_PASS;
        c0 = counters[4 * (size_t)b], c1 = counters[4 * (size_t)b + 1];
        c2 = counters[4 * (size_t)b + 2], c3 = counters[4 * (size_t)b + 3];
        if (q == 0) L.mv[p] = BKT_MOVE_NONE;
    }
    int played = 0, st_or = 0, ply = 0;
    for (;; ++ply) {                                                 // round `ply` selects ply `ply`; the body before it
        __syncthreads();                                             // plays ply `ply - 1` (round 0: no move, the start sets)
        play_one_ply(pos, B, over, &L);
        if (live && q == 0) st_or |= L.st[p];
        if (ply == max_plies) break;
        if (!__syncthreads_or(live && !done)) break;                 // (the barrier also publishes L.playable)
        const bool mine = live && !done && L.playable[NN * pp + q] != 0;
        const unsigned long long bal = __ballot(mine);
        if ((tid & 63) == 0) {
            sel[2 * (tid >> 6)] = (unsigned)bal;
            sel[2 * (tid >> 6) + 1] = (unsigned)(bal >> 32);
        }
        __syncthreads();
        if (live) {
            const BB P = position_set(sel, pp);
            const unsigned n = (unsigned)popc(P);
            const unsigned idx = ((philox4x32_10_x0(c0, c1 + (uint32_t)ply, c2, c3, k0, k1) >> 8) * n) >> 24;
            const unsigned rank = (k > 0 ? __popc(P.w[0]) : 0) + (k > 1 ? __popc(P.w[1]) : 0) + __popc(word_of(P, k) & below);
            int mv = BKT_MOVE_NONE - 1;                              // not this thread's to write
            if (done || n == 0) { if (q == 0) mv = done ? BKT_MOVE_NONE : BK_PASS; }
            else if (mine && rank == idx) mv = q;
            if (mv >= BKT_MOVE_NONE) {
                L.mv[p] = mv;
                if (hist) hist[(size_t)b * max_plies + ply] = (int16_t)mv;
            }
            if (!done) {                                             // every thread of the row knows the move
                const bool pass = n == 0;
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
    if (hist)                                                        // the plies this workgroup did not run
        for (int i = ply + q; i < max_plies; i += NN) hist[(size_t)b * max_plies + i] = (int16_t)BKT_MOVE_NONE;
}

}  // namespace

extern "C" int bkt_random_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, int max_plies, uint8_t* over,
                                   int32_t* plies, int16_t* moves, int32_t* status, void* stream) {
    if (!pos || !counters || !over || !plies || !status || batch < 1 || batch > BKT_MAX_BATCH || max_plies < 1 ||
        max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(random_playouts_kernel, dim3((batch + PPW - 1) / PPW), dim3(256), 0, (hipStream_t)stream,
                       static_cast<unsigned char*>(pos), batch, (uint32_t)seed, (uint32_t)(seed >> 32), counters, max_plies,
                       over, plies, moves, status);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

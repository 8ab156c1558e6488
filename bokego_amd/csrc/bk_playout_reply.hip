// bk_playout_reply.hip -- included as text at the end of bk_playout_pat.hip, after bk_playout_tac.hip (it is no translation
// unit of its own): the last-good-reply playouts of bokego_amd/rollout.py (include/bokego_train.h has the two rules; DESIGN
// 24).  bkt_reply_playouts is bkt_tactical_playouts whose draw asks a reply table first (ReplyDraw around WeightedDraw, or
// around the uniform draw when there is no table to weigh with); bkt_reply_update folds the histories of a batch of playouts
// and their winners back into that table, in two launches: reply_summaries_kernel, one workgroup per record, and
// the apply launch (reply_apply), one workgroup per table.  bkt_reply_playouts_tables and bkt_reply_update_tables are the same two for
// many tables at once -- a table per game of a self-play batch, named per row by `slots`.  One table is the case
// "every row uses table 0": the same draw with one staged table instead of one per seat of the workgroup, and the same apply
// body with one workgroup and no slots to test.

namespace {

constexpr int REPLY_ENTRIES = 2 * NN;                                // replies[colour][previous move]
constexpr int REPLY_WORDS = 4;                                       // a summary: three words of F, then set << 8 | value

// The tactical weight with either table optional: a NULL tactics table is 256 everywhere, which with a pattern table gives
// bkt_pattern_playouts' weights and without one a constant, bkt_random_playouts' draw (bk_playout_tac.hip).  Its LDS and its
// two __noinline__ helpers are TacticalWeight's.
struct OptionalTacticalWeight {
    const uint16_t* __restrict__ table;
    const uint16_t* __restrict__ tactics;
    __device__ __forceinline__ void stage(int tid) const {
        if (tid < BKT_TACTIC_ENTRIES) TacticalWeight::lds()->tactics[tid] = tactics ? tactics[tid] : (uint16_t)256;
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        play_one_ply_planes(pos, B, over, L, TacticalWeight::lds());
    }
    __device__ __forceinline__ unsigned operator()(const PatLds* W, int pp, int q, int lm, bool white_to_move) const {
        return tactical_weight(W, TacticalWeight::lds(), table, pp, q, lm, white_to_move);
    }
};

// The uniform draw with what the reply draw asks of its inner draw: the last move and the turn on entry, carried in registers
// as WeightedDraw carries them (L.mv still holds the move the body has just played when publish() begins, and is written
// again only behind publish()'s barrier).
struct TrackedUniformDraw {
    UniformDraw inner;
    int lm, turn0;
    __device__ __forceinline__ void start(Seat s, int last_move, int turn) {
        lm = last_move, turn0 = turn;
        inner.start(s, last_move, turn);
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds& L, bool mine, int played) {
        const int just = L.mv[s.pp];
        if (just > BKT_MOVE_NONE) lm = just;
        inner.publish(s, L, mine, played);
    }
    __device__ __forceinline__ unsigned total(Seat s) { return inner.total(s); }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned n) const { return inner.picks(r24, n); }
};

// The fourth draw: the inner draw, overruled by a reply table.  start() stages SEATS tables of 162 bytes in LDS, published
// by the ply loop's first barrier.  SEATS == 1: the one table at `replies`, which every row uses; slots, tables and B are
// not read.  SEATS == PPW: a table per seat, the one of that seat's row (replies + 162 * slot; 255 everywhere for a seat
// without a row or a slot outside 0..tables-1 -- the slot is compared before it indexes), in two rounds of the workgroup.
// publish() is the inner one's -- its last barrier is already behind the thread when the reply is looked up, so no barrier
// is added: the side to move and the last move are the registers the inner draw carries, the entry is one LDS byte of the
// seat's table that every thread of a row reads at the same address, and whether it is playable is one byte of the set
// play_body left in L.playable, which nothing writes before the next play().  An entry is compared (<= 80) before it
// indexes.  Every branch here is per thread and reaches no barrier.  A row that is over, or has no playable point, never
// gets here with a reply: the loop asks picks() only when total() > 0, and a reply in P makes the total positive.
template <class Inner, int SEATS>
struct ReplyDraw {
    Inner inner;
    const uint8_t* __restrict__ replies;
    const int32_t* __restrict__ slots;
    int tables, B;
    int q, reply;
    static constexpr int STRIDE = REPLY_ENTRIES + 2;
    static __device__ __forceinline__ uint8_t* lds() {
        __shared__ uint8_t table[SEATS * STRIDE];
        return table;
    }
    __device__ __forceinline__ void start(Seat s, int last_move, int turn) {
        if (SEATS == 1) {
            if (s.tid < REPLY_ENTRIES) lds()[s.tid] = replies[s.tid];
        } else {
            for (int i = s.tid; i < SEATS * REPLY_ENTRIES; i += 256) {    // two rounds: 486 entries
                const int seat = i / REPLY_ENTRIES, e = i - REPLY_ENTRIES * seat;
                const int row = (int)blockIdx.x * PPW + seat;
                const int slot = row < B ? slots[row] : -1;
                lds()[STRIDE * seat + e] = slot >= 0 && slot < tables ? replies[(size_t)slot * REPLY_ENTRIES + e] : (uint8_t)BKT_REPLY_NONE;
            }
        }
        q = s.q;
        inner.start(s, last_move, turn);
    }
    __device__ __forceinline__ void play(unsigned char* pos, int B_, unsigned char* over, PlyLds* L) const {
        inner.play(pos, B_, over, L);
    }
    __device__ __forceinline__ void publish(Seat s, const PlyLds& L, bool mine, int played) {
        inner.publish(s, L, mine, played);
        const int lm = inner.lm;                                     // the move before this ply: the inner draw keeps it
        reply = -1;
        if (lm >= 0 && lm < NN) {
            const int r = lds()[(SEATS == 1 ? 0 : STRIDE * s.pp) + (((inner.turn0 + played) & 1) ? NN : 0) + lm];
            if (r < NN && L.playable[NN * s.pp + r] != 0) reply = r;
        }
    }
    __device__ __forceinline__ unsigned total(Seat s) { return inner.total(s); }
    __device__ __forceinline__ bool picks(uint32_t r24, unsigned S) const {
        return reply >= 0 ? q == reply : inner.picks(r24, S);
    }
};

__global__ void __launch_bounds__(256) reply_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                             const uint32_t* __restrict__ counters,
                                                             const uint16_t* __restrict__ table,
                                                             const uint16_t* __restrict__ tactics,
                                                             const uint8_t* __restrict__ replies, int max_plies,
                                                             unsigned char* over, int32_t* __restrict__ plies,
                                                             int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<WeightedDraw<OptionalTacticalWeight>, 1>{{{table, tactics}}, replies});
}

// With neither table the inner draw is the uniform one: bkt_random_playouts' kernel and its cost, not the tactical kernel's
// with two neutral tables (the same games either way; DESIGN 24 has the times).
__global__ void __launch_bounds__(256) reply_uniform_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                     const uint32_t* __restrict__ counters,
                                                                     const uint8_t* __restrict__ replies, int max_plies,
                                                                     unsigned char* over, int32_t* __restrict__ plies,
                                                                     int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    __shared__ unsigned sel[8];
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<TrackedUniformDraw, 1>{{UniformDraw{sel}, 0, 0}, replies});
}

// The same two with a table per row: slots[i] names the table of row i among `tables`.

__global__ void __launch_bounds__(256) reply_tables_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                    const uint32_t* __restrict__ counters,
                                                                    const uint16_t* __restrict__ table,
                                                                    const uint16_t* __restrict__ tactics,
                                                                    const uint8_t* __restrict__ replies, int tables,
                                                                    const int32_t* __restrict__ slots, int max_plies,
                                                                    unsigned char* over, int32_t* __restrict__ plies,
                                                                    int16_t* __restrict__ hist, int32_t* __restrict__ status) {
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<WeightedDraw<OptionalTacticalWeight>, PPW>{{{table, tactics}}, replies, slots, tables, B});
}

__global__ void __launch_bounds__(256) reply_tables_uniform_playouts_kernel(unsigned char* pos, int B, uint32_t k0, uint32_t k1,
                                                                            const uint32_t* __restrict__ counters,
                                                                            const uint8_t* __restrict__ replies, int tables,
                                                                            const int32_t* __restrict__ slots, int max_plies,
                                                                            unsigned char* over, int32_t* __restrict__ plies,
                                                                            int16_t* __restrict__ hist,
                                                                            int32_t* __restrict__ status) {
    __shared__ unsigned sel[8];
    playouts(pos, B, k0, k1, counters, max_plies, over, plies, hist, status,
             ReplyDraw<TrackedUniformDraw, PPW>{{UniformDraw{sel}, 0, 0}, replies, slots, tables, B});
}

constexpr int REPLY_WAVES = 4;                                       // rows staged per barrier round
constexpr int REPLY_ROW = BKT_MAX_PLAYOUT_PLIES;

// The first launch of bkt_reply_update.  One workgroup per record r; thread e < 162 owns the table entry e = 81 c + prev
// and scans ALL of the record's rows in ascending order -- the fold is sequential in the rows, so unlike
// amaf_counts_sides_kernel, whose staging this is, a row is not one wave's: the rows of a round are staged by the whole
// workgroup (coalesced 2-byte loads, padded with BKT_MOVE_NONE to a multiple of 4 entries), and after ONE barrier every
// thread walks them one after the other by 8-byte LDS reads at the same address in all lanes (a broadcast), so the walk and
// its end at the first entry <= BKT_MOVE_NONE or at max_plies are workgroup-uniform.  Two buffers alternate: a round costs
// one barrier.  What the segment of events of these rows does to the entry is kept in registers as a summary:
//   F      the points m "forgotten" (a loser's reply m) before the first "set" of the segment, an 81-bit mask;
//   set, v whether a winner's reply was stored, and the value after the segment if so (a point, or 255 when forgotten again).
// Applied to an entry x: x = (x in F ? 255 : x), then x = v if set.  The summary of events A followed by events B is
// (A.set ? A.F : A.F | B.F;  A.set | B.set;  B.set ? B.v : A.v in B.F ? 255 : A.v): associative, which is what lets the
// records be scanned by different workgroups and composed in order by the second launch.  The four words of entry e go to
// scratch[(r * 4 + j) * 162 + e] with plain stores.  Integers only, no atomics, nothing waits on another workgroup; loop
// bounds and barriers depend on `playouts` and `max_plies` alone.  An entry of `moves` is only compared, never an index.
__global__ void __launch_bounds__(64 * REPLY_WAVES) reply_summaries_kernel(const unsigned char* __restrict__ pos,
                                                                          const int16_t* __restrict__ moves, int max_plies,
                                                                          const uint8_t* __restrict__ won, int playouts,
                                                                          uint32_t* __restrict__ scratch) {
    __shared__ __attribute__((aligned(8))) int16_t rows[2][REPLY_WAVES][REPLY_ROW];
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * playouts;                 // the record's first row
    const int padded = (max_plies + 3) & ~3;                           // <= REPLY_ROW
    const unsigned char* rec = pos + (size_t)blockIdx.x * BK_POS_BYTES;
    const int lm0 = (short)(*reinterpret_cast<const unsigned*>(rec + OFF_KO) >> 16);
    const int c0 = *reinterpret_cast<const int*>(rec + OFF_TURN) & 1;  // the colour to move at the record: 0 black, 1 white
    const int my_c = tid / NN, my_prev = tid < REPLY_ENTRIES ? tid - NN * my_c : -100;   // -100: equals no previous move
    uint32_t f0 = 0, f1 = 0, f2 = 0;
    bool set = false;
    int v = BKT_REPLY_NONE;
    int buf = 0;
    for (int j0 = 0; j0 < playouts; j0 += REPLY_WAVES, buf ^= 1) {
        const int here = min(REPLY_WAVES, playouts - j0);
        const int16_t* src = moves + (row0 + j0) * max_plies;
        for (int i = tid; i < padded; i += 64 * REPLY_WAVES) {          // the round's loads first: REPLY_WAVES in flight per thread
            int16_t e[REPLY_WAVES];
#pragma unroll
            for (int w = 0; w < REPLY_WAVES; ++w)
                e[w] = w < here && i < max_plies ? src[(size_t)w * max_plies + i] : (int16_t)BKT_MOVE_NONE;
#pragma unroll
            for (int w = 0; w < REPLY_WAVES; ++w) rows[buf][w][i] = e[w];
        }
        __syncthreads();
        for (int w = 0; w < here; ++w) {                               // in row order: uniform in the workgroup
            const bool win = won[row0 + j0 + w] != 0;                  // the side to move at the record won the row
            const int16_t* row = rows[buf][w];
            int prev = lm0;
            bool live = true;
            for (int k = 0; k < padded && live; k += 4) {
                const uint2 x = *reinterpret_cast<const uint2*>(row + k);
                const int m[4] = {(int16_t)(x.x & 0xFFFFu), (int16_t)(x.x >> 16), (int16_t)(x.y & 0xFFFFu), (int16_t)(x.y >> 16)};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    live = live && m[e] > BKT_MOVE_NONE;
                    // ply k + e has the parity of e (k is a multiple of 4): its mover's colour, and whether the mover won
                    const bool event = live && m[e] >= 0 && m[e] < NN && prev == my_prev && (c0 ^ (e & 1)) == my_c;
                    const bool mover_won = win == ((e & 1) == 0);
                    if (event && mover_won) set = true, v = m[e];
                    else if (event && set) v = v == m[e] ? BKT_REPLY_NONE : v;
                    else if (event) {
                        const uint32_t bit = 1u << (m[e] & 31);
                        f0 |= m[e] < 32 ? bit : 0u, f1 |= m[e] >= 32 && m[e] < 64 ? bit : 0u, f2 |= m[e] >= 64 ? bit : 0u;
                    }
                    prev = m[e];
                }
            }
        }
    }
    if (tid < REPLY_ENTRIES) {
        uint32_t* out = scratch + (size_t)blockIdx.x * REPLY_WORDS * REPLY_ENTRIES + tid;
        out[0] = f0, out[REPLY_ENTRIES] = f1, out[2 * REPLY_ENTRIES] = f2;
        out[3 * REPLY_ENTRIES] = (set ? 256u : 0u) | (uint32_t)(v & 255);
    }
}

// The second launch: workgroup t owns table t, and thread e < 162 applies to replies[t][e], in ascending record order, the
// summaries of the records whose slot is t: a chain of selects with a test in front of it.  SLOTS == false: every record
// belongs to the table, slots is not read, and the launch is one workgroup.  The test reads slots[r], the same word in every
// thread (uniform, and independent of the entry's value, so it and the loads behind it run ahead of the selects).  A value
// above 80 is in no F.  A table no record names is read and written back unchanged; a slot outside 0..tables-1 equals no
// workgroup's index, so such a record updates nothing.  One writer per byte, no workgroup reads what another writes: the
// result is the sequential fold whatever the scheduling.  (The test is a template parameter because a test of the pointer
// at run time, in one kernel for both, measured 10 us slower over 1,536 records with many tables: DESIGN 25.)
template <bool SLOTS>
__device__ __forceinline__ void reply_apply(const uint32_t* __restrict__ scratch, int records,
                                            const int32_t* __restrict__ slots, uint8_t* __restrict__ replies) {
    const int tid = threadIdx.x;
    if (tid >= REPLY_ENTRIES) return;
    const int t = (int)blockIdx.x;
    uint8_t* mine = replies + (size_t)t * REPLY_ENTRIES + tid;
    unsigned x = *mine;
    for (int r = 0; r < records; ++r) {
        if (SLOTS && slots[r] != t) continue;
        const uint32_t* in = scratch + (size_t)r * REPLY_WORDS * REPLY_ENTRIES + tid;
        const uint32_t f0 = in[0], f1 = in[REPLY_ENTRIES], f2 = in[2 * REPLY_ENTRIES], sv = in[3 * REPLY_ENTRIES];
        const uint32_t word = x < 32u ? f0 : x < 64u ? f1 : f2;
        if (x < (unsigned)NN && (word >> (x & 31u) & 1u)) x = BKT_REPLY_NONE;
        if (sv & 256u) x = sv & 255u;
    }
    *mine = (uint8_t)x;
}

__global__ void __launch_bounds__(192) reply_apply_kernel(const uint32_t* __restrict__ scratch, int records,
                                                          uint8_t* __restrict__ replies) {
    reply_apply<false>(scratch, records, nullptr, replies);
}

__global__ void __launch_bounds__(192) reply_slots_apply_kernel(const uint32_t* __restrict__ scratch, int records,
                                                                const int32_t* __restrict__ slots,
                                                                uint8_t* __restrict__ replies) {
    reply_apply<true>(scratch, records, slots, replies);
}

// What the two playout entry points share: slots == nullptr is the single table (tables is then 1), and with neither weight
// table the inner draw is the uniform one.
int reply_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table, const uint16_t* tactics,
                   const uint8_t* replies, int tables, const int32_t* slots, int max_plies, uint8_t* over, int32_t* plies,
                   int16_t* moves, int32_t* status, void* stream) {
    if (!replies || tables < 1 || tables > BKT_MAX_BATCH) return BKT_ERR_ARG;
    const auto launch = [&](auto kernel, auto... extra) {
        return launch_playouts(kernel, pos, batch, seed, counters, max_plies, over, plies, moves, status, stream, extra...);
    };
    if (!table && !tactics)
        return slots ? launch(reply_tables_uniform_playouts_kernel, replies, tables, slots)
                     : launch(reply_uniform_playouts_kernel, replies);
    return slots ? launch(reply_tables_playouts_kernel, table, tactics, replies, tables, slots)
                 : launch(reply_playouts_kernel, table, tactics, replies);
}

// What the two update entry points share: the summaries of the records, then a workgroup per table (slots == nullptr: one,
// tables is then 1).
int reply_update(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records, int playouts,
                 uint8_t* replies, int tables, const int32_t* slots, void* scratch, void* stream) {
    if (!pos || !moves || !won || !replies || !scratch || records < 1 || playouts < 1 || tables < 1 ||
        tables > BKT_MAX_BATCH || (int64_t)records * playouts > BKT_MAX_SAMPLE_ROWS || max_plies < 1 ||
        max_plies > BKT_MAX_PLAYOUT_PLIES)
        return BKT_ERR_ARG;
    hipLaunchKernelGGL(reply_summaries_kernel, dim3(records), dim3(64 * REPLY_WAVES), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(pos), moves, max_plies, won, playouts, static_cast<uint32_t*>(scratch));
    if (hipGetLastError() != hipSuccess) return BKT_ERR_HIP;
    if (slots)
        hipLaunchKernelGGL(reply_slots_apply_kernel, dim3(tables), dim3(192), 0, (hipStream_t)stream,
                           static_cast<const uint32_t*>(scratch), records, slots, replies);
    else
        hipLaunchKernelGGL(reply_apply_kernel, dim3(1), dim3(192), 0, (hipStream_t)stream,
                           static_cast<const uint32_t*>(scratch), records, replies);
    return hipGetLastError() == hipSuccess ? BKT_OK : BKT_ERR_HIP;
}

}  // namespace

extern "C" int bkt_reply_playouts(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                  const uint16_t* tactics, const uint8_t* replies, int max_plies, uint8_t* over,
                                  int32_t* plies, int16_t* moves, int32_t* status, void* stream) {
    return reply_playouts(pos, batch, seed, counters, table, tactics, replies, 1, nullptr, max_plies, over, plies, moves, status,
                          stream);
}

extern "C" size_t bkt_reply_scratch_bytes(int records) {
    return records < 1 ? 0 : (size_t)records * REPLY_WORDS * REPLY_ENTRIES * sizeof(uint32_t);
}

extern "C" int bkt_reply_update(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records,
                                int playouts, uint8_t* replies, void* scratch, void* stream) {
    return reply_update(pos, moves, max_plies, won, records, playouts, replies, 1, nullptr, scratch, stream);
}

extern "C" int bkt_reply_playouts_tables(void* pos, int batch, uint64_t seed, const uint32_t* counters, const uint16_t* table,
                                         const uint16_t* tactics, const uint8_t* replies, int tables, const int32_t* slots,
                                         int max_plies, uint8_t* over, int32_t* plies, int16_t* moves, int32_t* status,
                                         void* stream) {
    if (!slots) return BKT_ERR_ARG;
    return reply_playouts(pos, batch, seed, counters, table, tactics, replies, tables, slots, max_plies, over, plies, moves,
                          status, stream);
}

extern "C" int bkt_reply_update_tables(const void* pos, const int16_t* moves, int max_plies, const uint8_t* won, int records,
                                       int playouts, uint8_t* replies, int tables, const int32_t* slots, void* scratch,
                                       void* stream) {
    if (!slots) return BKT_ERR_ARG;
    return reply_update(pos, moves, max_plies, won, records, playouts, replies, tables, slots, scratch, stream);
}

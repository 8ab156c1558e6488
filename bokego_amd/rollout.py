"""Play positions out to the end of the game on the device and score the settled boards.

    python -m bokego_amd.rollout --sgf FILE [--move K] -p POLICY [-n 256] [--seed S] [--komi 5.5] [--device D]

finish_games plays every record on, both colours, until two passes in a row end the game: the side to move samples from
the policy (or uniformly, engine=None) among its *playable* points -- legal, and not its own one-point eye as the
reference's go.possible_eye defines one -- and passes when it has none.  Neither side can then destroy its own living
groups, so dead stones get captured, open regions get filled, and the raw Tromp-Taylor area of the final board
(bkt_area_score) is the result of the game.  rollout_score averages n such playouts per position into a score, an
ownership map and the status (alive / dead / seki) of every stone, which is what the reference asks GNU Go for.

Lock-step on the device.  One bkt_playout_step with every move BKT_MOVE_NONE gives the planes and the playable sets of
the start records; then per ply LeafEngine.eval_device (logits), bkt_sample_moves_masked on the playable set, one write
into the device move history, and bkt_playout_step, which plays the move or the pass, keeps the `over` flag of a game
that has ended and writes the next planes and playable set.  No host work, download or synchronisation per ply: the
host looks at `over` once every CHECK_EVERY plies and stops when every game is over, or at max_plies.  Simple ko only:
a game can cycle, and the cap is what ends it; it is then scored as it stands and counted in `unfinished`.

Randomness is Philox4x32-10 keyed by the seed with a counter per game and ply, never per row: by default
(g mod 2^32, the record's turn + plies played here, g >> 32, STREAM_ROLLOUT) -- lockstep.py has the table of streams,
which keeps these draws apart from genvals' -- or the caller's own layout (counters=) whose second word runs on with
the ply.

random_playouts is the engine=None case without the lock-step: no network sits between two plies, so ONE launch
(bkt_random_playouts) plays every game to its end, each workgroup looping over the plies of its three records (DESIGN
16).  Its choice among the n playable points is integer arithmetic on the Philox word -- the ((x0 >> 8) * n) >> 24-th
point in ascending order -- so the host mirror (rules="host") equals the device bit for bit, with no margin to excuse.
playout_value turns it into the classical Monte-Carlo value of a position, the share of n such playouts the side to
move wins, and PlayoutEvaluator hands that value to the tree search in place of a value net (priors from the policy).

    python -m bokego_amd.rollout --sgf FILE [--move K] --random [--patterns FILE] [--tactics FILE] [-n 256] [--seed S]   # one launch

patterns= (a patterns.PatternTable; --patterns FILE) draws those moves in proportion to 3x3 pattern weights instead
(bkt_pattern_playouts; bokego_amd/patterns.py): opt-in, and with patterns=None every call is what it was.
tactics= (a tactics.TacticTable; --tactics FILE) multiplies those weights -- or, without patterns, a constant -- by the
capture / escape / atari weight of each point's tactical code (bkt_tactical_playouts; bokego_amd/tactics.py):
opt-in likewise, and with tactics=None the same launches run as before.

playout_amaf keeps what those playouts otherwise throw away: beside the value, for every point the number of playouts in
which the side to move was the first to play it and the number of those it won -- the all-moves-as-first (AMAF) counts,
one bkt_amaf_counts reduction over the playouts' move history.  amaf_prior turns them into a search prior, and
PlayoutEvaluator(prior=1.0) into an engine that searches with no network at all.

    python -m bokego_amd.rollout --sgf FILE [--move K] --random --amaf [-n 256]   # the value and the heaviest prior moves

playout_amaf(sides=2) keeps the opponent's half of every history too (one bkt_amaf_counts_sides), and
PlayoutEvaluator(rave=True) hands those two-sided counts of every row to the tree, whose RAVE tables are made of them
(bk_pool_deliver_rave, NativeMCTS(playout_rave=k)).  `--amaf --sides 2` prints both sides' heaviest points.

playout_ownership keeps the other thing a playout leaves behind, the final board: one bkt_owner_counts scores the final
records of every record's n playouts and reduces them, in that launch, to integer counts -- how often each point ended up
black's, white's and the winner's, the playouts by their margin, black's wins -- without an owner array ever reaching
memory.  Ownership carries them: the mean ownership map, the mean margin and Coulom's criticality, which
amaf_prior(criticality=, gamma=) and PlayoutEvaluator(criticality=gamma) can add to the prior (opt-in, untuned).

    python -m bokego_amd.rollout --sgf FILE [--move K] --random --ownership [-n 256]   # the owner board and the critical points

move_weights asks the playouts' move predictor itself: the weight the tactical draw gives every point of a record at the
first ply, in one launch (bkt_move_weights).  pattern_prior is that table's own prediction, and
amaf_prior(weights=, mu=) and PlayoutEvaluator(pattern_prior=mu) add mu * ln(weight) to the prior's logits -- Coulom's
pattern ratings, or progressive bias, seeding a new node (opt-in, untuned).

    python -m bokego_amd.rollout --sgf FILE [--move K] --random --weights [--patterns FILE] [--tactics FILE]   # the ten heaviest points

replies= (a ReplyTable, bokego_amd/replies.py) lets those playouts learn from each other: the last-good-reply policy with
forgetting.  The table holds, per colour and previous move, the reply that last won a playout; a playout plays
it where it is playable (bkt_reply_playouts), and after the score one bkt_reply_update stores the winners' replies of the
batch and takes the losers' out.  playout_value, playout_amaf and random_playouts update the table they are given in place;
PlayoutEvaluator(replies=True) keeps one across the requests of a search (opt-in, untuned).  A ReplyTable2 in its place keys
the replies by the last two moves, with that table as its plane 81 and fallback (bkt_reply2_playouts, bkt_reply2_update;
DESIGN 26); PlayoutEvaluator(replies=2) keeps one.  A ReplyTables2 with slots= is a pair table per game of a batch
(bkt_reply2_playouts_tables, bkt_reply2_update_tables); PlayoutEvaluator(pair_games=G) keeps G of them.

    python -m bokego_amd.rollout --sgf FILE [--move K] --random --replies [-n 256] [--chunk 16]   # the share of plies the table decided
    python -m bokego_amd.rollout --sgf FILE [--move K] --random --reply-pairs [-n 256] [--chunk 16]   # the same with a ReplyTable2:
                                                                          # replies keyed by the last two moves

move_values= (a MoveValueTable, bokego_amd/movevalues.py) is the soft counterpart (MAST): a win rate per colour
and point, learned from the same histories and multiplied into the draw's weights (bkt_move_value_playouts,
bkt_move_value_update), alone or under either reply table; PlayoutEvaluator(move_values=True) keeps one (opt-in, untuned).
A movevalues.MoveValueTables with slots= is a move-value table per game of a batch (bkt_move_value_playouts_tables,
bkt_move_value_update_tables), alone or beside a ReplyTables or a ReplyTables2 named by the same slots;
PlayoutEvaluator(move_value_games=G) keeps G of them.
A movecontexts.MoveContextTable as move_values= keys the same factor by the previous move as well (NAST): its
plane 81 is the move-value table, the calls are bkt_move_context_playouts and bkt_move_context_update, alone or under
a ReplyTable or a ReplyTable2 and never with slots=; PlayoutEvaluator(move_contexts=True) keeps one (opt-in, untuned).

    python -m bokego_amd.rollout --sgf FILE [--move K] --random --move-values [-n 256] [--chunk 16]   # what the table learned

rules="host" is one loop (_playout_host) on the host rules with the same draws (lockstep's play_host, features_batch
and area_score_host, bk_pos_is_legal, bk_pos_possible_eye, lockstep.sample_host in float64): the reference the tests
compare the device with.  With engine=None it needs no GPU.
"""
import argparse
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import torch

from . import _trainlib as T
from . import go
from . import lockstep as L
from .lockstep import playable_host, record_turns  # noqa: F401  (public here: see __all__)
from .movevalues import DEFAULT_TAU, MoveValueTable, MoveValueTables, move_value_update_host, move_value_weights
from .movecontexts import MoveContextTable, move_context_update_host, move_context_weights
from .replies import (ReplyTable, ReplyTable2, ReplyTables, ReplyTables2, reply2_moves, reply2_plies_of, reply2_update_host, reply_moves, reply_plies_of,
                      reply_update_host, slots_of)

MAX_PLIES = 400            # default cap of finish_games: 2.8x the longest playout measured (142 plies)
CHECK_EVERY = 16           # plies between two looks at `over`
MOVE_NONE = -2             # BKT_MOVE_NONE; in the history: the game was over before this ply
SEKI_THRESHOLD = 0.5       # |mean ownership| of a stone's point below this: the stone is in seki (rollout_score)
POS_BYTES = L.POS_BYTES

__all__ = ["MAX_PLIES", "MOVE_NONE", "Amaf", "Finished", "Ownership", "PlayoutEvaluator", "ReplyTable", "ReplyTable2", "ReplyTables", "ReplyTables2", "RolloutScore",
           "amaf_counts_host", "reply_update_host", "reply2_update_host", "reply_pairs_report",
           "amaf_counts_sides_host", "amaf_prior",
           "default_counters", "finish_games", "format_score", "move_weights", "move_weights_host", "owner_board",
           "ownership_score", "reply_report", "owner_counts_host", "owner_host", "pattern_prior",
           "playable_host", "playout_amaf", "playout_ownership",
           "playout_value", "random_playouts", "record_turns", "rollout_score", "sgf_position"]


class Finished:
    """What finish_games returns, rows in the order of `pos`.

    records     uint8 [G,192]   the final bk_pos records (a device tensor with rules="device", numpy with "host")
    moves       int16 [G,L]     (numpy) the move at each ply played here: a point, -1 = pass, -2 = the game was over;
                                L = the longest game
    over        bool [G]        two passes in a row ended the game
    plies       int64 [G]       plies played here, the two passes included
    score       float32 [G]     area score of the final record (black - (white + komi))
    owner       int8 [G,81]     +1 black stone or black-only region, -1 white, 0 neither
    unfinished  int             rows not over at the cap
    min_margin  float64 [G]     rules="host" only: the smallest lockstep.cdf_margin among the game's draws
    reply_plies int or None     random_playouts(replies=): the plies the reply table decided (rules="host"; None on the device)
    reply_pair_plies            with a ReplyTable2: those of them its pair entries decided (likewise); None with any other table
    """


def default_counters(n, turns):
    """(g mod 2^32, turn, g >> 32, 2) for the games g = 0 .. n-1, int32 [n, 4]."""
    return L.game_counters(np.arange(n, dtype=np.uint64), turns, L.STREAM_ROLLOUT)


def _engines(engine, sides, G):
    """-> (None | one engine | (a, b), n0)."""
    if isinstance(engine, (tuple, list)):
        if len(engine) != 2 or sides is None or len(sides) != 1:
            raise ValueError("the pair form is engine=(engine_black, engine_white) with sides=(n0,)")
        n0 = int(sides[0])
        if not 0 <= n0 <= G:
            raise ValueError(f"sides[0] must be 0..{G}, got {n0}")
        return tuple(engine), n0
    if sides is not None:
        raise ValueError("sides goes with the pair form engine=(engine_black, engine_white)")
    return engine, G


def _check_records(pos):
    if tuple(pos.shape[1:]) != (POS_BYTES,) or pos.ndim != 2 or (str(pos.dtype) not in ("uint8", "torch.uint8")):
        raise ValueError(f"pos must be uint8 [G, {POS_BYTES}], got {pos.dtype} {tuple(pos.shape)}")
    if len(pos) < 1:
        raise ValueError("pos holds no record")


def _numpy(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _device(device, eng=None, pos=None):
    """The device of a call: `device` when given, else the engine's, else that of the records, else the current one."""
    if device is not None:
        return torch.device(device)
    if eng is not None:
        return torch.device("cuda", (eng[0] if isinstance(eng, tuple) else eng).device_id)
    if isinstance(pos, torch.Tensor) and pos.is_cuda:
        return pos.device
    return torch.device("cuda", torch.cuda.current_device())


def _pairs(eng, planes, black_to_move, n0):
    """The (engine, rows) L.engine_logits takes: one engine for all rows, or the pair -- rows [0, n0) by the first engine
    when black is to move, by the second when white is; rows [n0, G) the other way round."""
    if not isinstance(eng, tuple):
        return [(eng, planes)]
    first, second = eng if black_to_move else eng[::-1]
    return [(first, planes[:n0]), (second, planes[n0:])]


def _finished(records, moves, plies, over, score, owner):
    """A Finished; moves: the whole history [G, max_plies] (numpy or a tensor), cut here to the longest game, or None."""
    out = Finished()
    out.records, out.plies, out.over, out.score, out.owner = records, plies, over, score, owner
    out.moves = None if moves is None else np.ascontiguousarray(_numpy(moves[:, :max(int(plies.max()), 1)]))
    out.unfinished = int((~over).sum())
    return out


def _check_status(status, verb):
    L.check_status(status, lambda s, st: f"row {s}: a {verb} move is illegal (status {st}); the playable set and the rules "
                   "disagree")


def finish_games(pos, engine, seed, counters=None, max_plies=MAX_PLIES, rules="device", device=None, sides=None,
                 komi=L.KOMI):
    """Play the records pos (uint8 [G,192], numpy or a tensor; not modified) to the end of the game -> Finished.

    engine: one fp32 LeafEngine with policy weights that plays both colours; None: uniform logits (random eye-safe
    playouts, no network); or the pair form (engine_black, engine_white) with sides=(n0,): in rows [0, n0) the first
    engine plays black and the second white, in rows [n0, G) the second plays black and the first white (the two
    slices of reinforce.play_games) -- every record must then have the same parity of turn (ValueError otherwise).
    counters: int32 [G,4] Philox counter words of the first ply; word 1 runs on with the ply.  Default: default_counters.
    """
    L.check_rules(rules)
    max_plies = int(max_plies)
    if max_plies < 1:
        raise ValueError("max_plies must be at least 1")
    _check_records(pos)
    G = len(pos)
    eng, n0 = _engines(engine, sides, G)
    turns = None
    if counters is None or isinstance(eng, tuple):
        turns = record_turns(_numpy(pos))
    black_first = True
    if isinstance(eng, tuple):
        if len(set((turns & 1).tolist())) != 1:
            raise ValueError("the pair form needs every record at the same parity of turn")
        black_first = int(turns[0]) % 2 == 0
    if counters is None:
        counters = default_counters(G, turns)
    key = L.seed_u64(seed)
    if rules == "host":
        return _finish_host(pos, eng, n0, black_first, key, L.counters_to_host(counters, G), max_plies, device, komi)
    return _finish_device(pos, eng, n0, black_first, key, counters, max_plies, device, komi)


def _finish_device(pos, eng, n0, black_first, key, counters, max_plies, device, komi):
    dev = _device(device, eng, pos)
    G = len(pos)
    if G > T.MAX_BATCH:
        raise ValueError(f"at most {T.MAX_BATCH} games per call, got {G}")
    pos = L.records_to_device(pos, dev)
    ctr = L.counters_to_device(counters, G, dev)
    planes = torch.empty((G, 27, 9, 9), dtype=torch.uint8, device=dev) if eng is not None else None
    playable = torch.empty((G, 81), dtype=torch.uint8, device=dev)
    over = torch.zeros((G,), dtype=torch.uint8, device=dev)
    none = torch.full((G,), MOVE_NONE, dtype=torch.int32, device=dev)
    hist = torch.full((G, max_plies), MOVE_NONE, dtype=torch.int16, device=dev)
    uniform = torch.zeros((G, 81), dtype=torch.float32, device=dev) if eng is None else None
    status = T.playout_step(pos, none, over, planes, playable)            # the start planes and playable sets
    for k in range(max_plies):
        if k:
            ctr[:, 1] += 1
            if k % CHECK_EVERY == 0 and bool(over.all()):                 # the only look at the device inside the loop
                break
        logits = uniform if eng is None else L.engine_logits(_pairs(eng, planes, black_first == (k % 2 == 0), n0))
        moves, _ = T.sample_moves_masked(logits, playable, key, ctr)
        moves = torch.where(over != 0, none, moves)
        hist[:, k] = moves
        status |= T.playout_step(pos, moves, over, planes, playable)
    score, owner = T.area_score(pos, komi, owner=True)
    moves = hist.cpu().numpy()
    _check_status(status, "sampled")
    return _finished(pos, moves, (moves > MOVE_NONE).sum(1).astype(np.int64), over.cpu().numpy() != 0,
                     score.cpu().numpy(), owner.cpu().numpy())


def _playout_host(pos, key, ctr, max_plies, komi, choose, verb, history=True):
    """The one host loop: play a copy of the records pos to two passes in a row (or max_plies) -> Finished.  Per ply, for
    the rows still live: their playable sets and one Philox draw each (ctr, word 1 running on with the ply), then
    choose(k, recs, live, playable, x0) -> the move of each live row (-1: pass)."""
    recs = np.array(_numpy(pos), np.uint8, order="C")
    over = np.zeros(len(recs), bool)
    hist = np.full((len(recs), max_plies), MOVE_NONE, np.int16)
    kw = L.seed_key(key)
    ctr = ctr.view(np.uint32).copy()
    for k in range(max_plies):
        if over.all():
            break
        if k:
            ctr[:, 1] += np.uint32(1)                                      # wraps at 2^32, as the kernels' c1 + k
        live = np.nonzero(~over)[0]
        mv = np.asarray(choose(k, recs, live, playable_host(recs[live]), L.philox4x32_10(ctr[live], kw)[:, 0]))
        hist[live, k] = mv
        over[live[(mv < 0) & (L.record_last_move(recs)[live] == go.PASS)]] = True
        L.play_host(recs, live, mv, lambda g, m: f"row {g}: {verb} move {m} is illegal; the playable set and the rules "
                    "disagree", liberties=True)
    return _finished(recs, hist if history else None, (hist > MOVE_NONE).sum(1).astype(np.int64), over,
                     L.area_score_host(recs, komi).astype(np.float32), owner_host(recs))


def _finish_host(pos, eng, n0, black_first, key, ctr, max_plies, device, komi):
    """finish_games on the host: the move is bkt_sample_moves_masked's, from the float64 CDF of the logits."""
    G = len(pos)
    margin = np.full(G, np.inf)
    if eng is not None:
        dev = _device(device, eng)
        feats = np.empty((G, 27, 9, 9), np.uint8)

    def choose(k, recs, live, ok, x0):
        if eng is None:
            logits = np.zeros((G, 81))
        else:                                                             # every row, so that the pair's slices stay put
            L.features_batch(recs, feats.ctypes.data)
            logits = L.engine_logits(_pairs(eng, torch.from_numpy(feats).to(dev), black_first == (k % 2 == 0), n0))
            logits = logits.cpu().numpy().astype(np.float64)
        u = L.uniform(x0)
        margin[live] = np.minimum(margin[live], L.cdf_margin(logits[live], u))
        return L.sample_host(logits[live], ok, u)[0]

    out = _playout_host(pos, key, ctr, max_plies, komi, choose, "sampled")
    out.min_margin = margin
    return out


def owner_host(recs):
    """bkt_area_score's owner on the host: int8 [n,81], +1 black stone or black-only empty region, -1 white, 0 neither."""
    out = np.zeros((len(recs), 81), np.int8)
    for i in range(len(recs)):
        b = recs[i, :81].view(np.int8)
        out[i] = np.where(b == 1, 1, np.where(b == 2, -1, 0))
        seen = np.zeros(81, bool)
        for s in range(81):
            if b[s] != 0 or seen[s]:
                continue
            region, stack, touch = [], [s], set()
            seen[s] = True
            while stack:
                q = stack.pop()
                region.append(q)
                for t in go.NEIGHBORS[q]:
                    if b[t] != 0:
                        touch.add(int(b[t]))
                    elif not seen[t]:
                        seen[t] = True
                        stack.append(t)
            if touch == {1}:
                out[i, region] = 1
            elif touch == {2}:
                out[i, region] = -1
    return out



# ---- whole random playouts in one launch, and the Monte-Carlo value ----------------------------------------------------------
def select_index(x0, n):
    """The rank, among n playable points in ascending order, that the Philox word x0 selects: ((x0 >> 8) * n) >> 24, in
    [0, n) for n >= 1 (and 0 for n = 0: the row passes).  24 x 7 bits: exact in 32-bit unsigned arithmetic on the device."""
    return ((np.asarray(x0, np.uint64) >> np.uint64(8)) * np.asarray(n, np.uint64)) >> np.uint64(24)



def _random_host(pos, key, ctr, max_plies, komi, history, table=None, tactics=None, replies=None, slots=None, move_values=None):
    """random_playouts on the host: the select_index-th playable point in ascending order, a pass when there is none; with
    a table (a patterns.PatternTable), patterns.select_weighted on the entries of the points' pattern indices; with tactics
    (a tactics.TacticTable), tactics.select_tactical on those entries (or none) and the entries of the tactical codes.
    replies (a ReplyTable or uint8 [2,81], read only here): the use rule of replies.py goes first -- where the table's reply
    to a row's last move is playable it is the move, whatever the draw above says; the Finished then carries reply_plies,
    the number of plies the table decided.  slots: with tables [count,2,81] (a ReplyTables), the table of every row.
    With a ReplyTable2 the use rule is reply2_moves': the move two plies back is kept per row across the plies here (none at
    ply 0, the record's last move at ply 1), and reply_pair_plies is the pair entries' share of reply_plies; with a
    ReplyTables2 likewise, slots naming the pair table of every row.
    move_values (a MoveValueTable, read only here): the weights of the draw above -- 256 everywhere without
    tables -- go through movevalues.move_value_weights with the values as they stand on entry and the colour to move; with a
    MoveValueTables, slots names the table of every row, the same slot as its reply table's; with a
    MoveContextTable they go through movecontexts.move_context_weights with the row's last move."""
    def choose(k, recs, live, ok, x0):
        n = ok.sum(1)
        pick = np.argmax(np.cumsum(ok, 1) > select_index(x0, n).astype(np.int64)[:, None], 1)
        return np.where(n > 0, pick, go.PASS)

    def choose_weighted(k, recs, live, ok, x0):
        return PT.select_weighted(x0, table.entries(PT.codes_host(recs[live])), ok)

    def choose_tactical(k, recs, live, ok, x0):
        part = recs[live]
        entries = None if table is None else table.entries(PT.codes_host(part))
        return TC.select_tactical(x0, entries, tactics.entries(TC.codes_host(part)), ok)

    def choose_valued(k, recs, live, ok, x0):
        part = recs[live]
        entries = None if table is None else table.entries(PT.codes_host(part))
        t = np.full(ok.shape, TC.NEUTRAL, np.uint16) if tactics is None else tactics.entries(TC.codes_host(part))
        if contexts:                                                      # keyed by the move played just before
            return PT.select_weighted(x0, move_context_weights(TC.combine(entries, t), values, record_turns(part) & 1,
                                                               L.record_last_move(part)), ok)
        return PT.select_weighted(x0, move_value_weights(TC.combine(entries, t), values, record_turns(part) & 1,
                                                         None if value_slots is None else value_slots[live]), ok)

    if table is not None or move_values is not None:
        from . import patterns as PT
    if tactics is not None or move_values is not None:
        from . import tactics as TC
    if move_values is not None:
        values, contexts = move_values.values.copy(), isinstance(move_values, MoveContextTable)
        value_slots = np.asarray(slots) if isinstance(move_values, MoveValueTables) else None   # the table of every row
        choose = choose_valued
    elif tactics is not None:
        choose = choose_tactical
    elif table is not None:
        choose = choose_weighted
    if replies is None:
        return _playout_host(pos, key, ctr, max_plies, komi, choose, "selected", history)
    decided, draw = [0, 0], choose
    pairs = isinstance(replies, _PAIRS)
    prev2 = np.full(len(pos), MOVE_NONE, np.int64)                        # per row: the move two plies back, none yet

    def choose(k, recs, live, ok, x0):                                    # noqa: F811  (the draw, overruled by the table)
        if pairs:
            r, which = reply2_moves(replies, recs[live], prev2[live], ok, None if slots is None else np.asarray(slots)[live])
            prev2[live] = L.record_last_move(recs[live])                  # every live row plays a move or passes now
            decided[1] += int((which == 2).sum())
        else:
            r = reply_moves(replies, recs[live], ok, None if slots is None else np.asarray(slots)[live])
        decided[0] += int((r >= 0).sum())
        return np.where(r >= 0, r, draw(k, recs, live, ok, x0))

    fin = _playout_host(pos, key, ctr, max_plies, komi, choose, "selected", history)
    fin.reply_plies = decided[0]
    fin.reply_pair_plies = decided[1] if pairs else None
    return fin


def _table(patterns):
    """patterns= of the callers below: None, a patterns.PatternTable, a uint16 array or a path -> None or a PatternTable."""
    if patterns is None:
        return None
    from .patterns import as_table
    return as_table(patterns)


def _tactics(tactics):
    """tactics= of the callers below: None, a tactics.TacticTable, a uint16 array or a path -> None or a TacticTable."""
    if tactics is None:
        return None
    from .tactics import as_tactics
    return as_tactics(tactics)


def random_playouts(pos, seed, counters=None, max_plies=MAX_PLIES, rules="device", komi=L.KOMI, history=True, device=None,
                    patterns=None, tactics=None, replies=None, slots=None, move_values=None):
    """Play the records pos (uint8 [G,192], numpy or a tensor; not modified) to the end of the game with uniformly random
    eye-safe moves -> Finished, the fields finish_games returns (moves is None with history=False; no min_margin: nothing
    is rounded).  rules="device": one bkt_random_playouts launch per T.MAX_BATCH rows, then bkt_area_score.  rules="host":
    the mirror on bk_pos_play / bk_pos_is_legal / bk_pos_possible_eye and lockstep.philox4x32_10; it needs no GPU and
    gives the same bits.  counters: int32 [G,4], the Philox counter words of ply 0 (word 1 runs on with the ply); default:
    default_counters, as finish_games.  A row's game depends on its record, the seed and its counters only.
    These are not finish_games(engine=None)'s games: that sampler goes through a float CDF.
    patterns: None, or a table of 3x3 pattern weights (patterns.PatternTable, or what patterns.as_table takes): the move is
    then drawn in proportion to the weights of the playable points (bkt_pattern_playouts), on the same words.
    tactics: None, or a table of tactical weights (tactics.TacticTable, or what tactics.as_tactics takes) that multiply the
    pattern weights, or a constant without patterns (bkt_tactical_playouts).
    replies: None, or a ReplyTable, which every game here reads as it stands (bkt_reply_playouts: where its reply to the
    last move is playable, that is the move) and which is then updated in place with all G games, rows ascending, each
    game a record of its own (bkt_reply_update).  The history is written whatever `history` says; black wins a
    game whose score is > 0.  The games then depend on the table too.
    slots: with a ReplyTables (a table per game of a batch), an int array [G], the table of every game: required
    with a ReplyTables and refused with a ReplyTable.  A ReplyTables2 takes them likewise (a pair table per game),
    and a ReplyTable2 refuses them.
    move_values: None, or a movevalues.MoveValueTable (MAST): every game here draws with the table's values as
    they stand multiplied into the weights (bkt_move_value_playouts, with replies= composed as above), and the table is
    then updated in place with all G games, after the reply table if any (bkt_move_value_update).  Not with slots=
    (TypeError): a MoveValueTable is one table for all games.  A movevalues.MoveValueTables (a table per game)
    needs slots= (TypeError without), alone or with a ReplyTables or a ReplyTables2 of the same count (ValueError), whose
    tables the same slots name; a single ReplyTable or ReplyTable2 is refused with it (TypeError).  A
    movecontexts.MoveContextTable (NAST) is a MoveValueTable keyed by the previous move as well: the same
    composition and the same refusal of slots=, on bkt_move_context_playouts and bkt_move_context_update."""
    L.check_rules(rules)
    table, tactics = _table(patterns), _tactics(tactics)
    slots = _check_tables(replies, move_values, slots, len(pos))
    learns = replies is not None or move_values is not None
    max_plies = int(max_plies)
    if not 1 <= max_plies <= 1024:
        raise ValueError("max_plies must be 1..1024 (BKT_MAX_PLAYOUT_PLIES)")
    _check_records(pos)
    G = len(pos)
    if counters is None:
        counters = default_counters(G, record_turns(_numpy(pos)))
    key = L.seed_u64(seed)
    if rules == "host":
        fin = _random_host(pos, key, L.counters_to_host(counters, G), max_plies, komi, history or learns, table,
                           tactics, replies, slots, move_values)
        if learns:
            start = np.asarray(_numpy(pos))                               # (moves is cut to the longest game: the same fold)
            won, moves = (fin.score > 0) == L.black_to_move(start), fin.moves
            if replies is not None:
                _update_host(replies, start, moves, won, G, 1, slots)
            if move_values is not None:
                _update_move_values_host(move_values, start, moves, won, G, 1, slots)
            fin.moves = moves if history else None
        return fin
    dev = _device(device, None, pos)
    start = L.records_to_device(pos, dev, clone=False)
    pos = start.clone()
    ctr = L.counters_to_device(counters, G, dev, clone=False)
    slots = _slots_device(slots, dev)
    over, plies, moves, status = _play_random_device(pos, key, ctr, max_plies, history or learns, table, tactics,
                                                     replies, slots, move_values)
    score, owner = _area_score_device(pos, komi, True)
    if learns:
        won = ((score > 0) == L.black_to_move(start)).to(torch.uint8)
        if replies is not None:
            _update_device(start, moves, won, G, 1, replies, slots)
        if move_values is not None:
            _update_move_values_device(start, moves, won, G, 1, move_values, slots)
    _check_status(status, "selected")
    fin = _finished(pos, moves if history else None, plies.cpu().numpy().astype(np.int64), over.cpu().numpy() != 0,
                    score.cpu().numpy(), owner.cpu().numpy())
    fin.reply_plies = fin.reply_pair_plies = None
    return fin


def _update_host(replies, recs, moves, won, records, playouts, slots):
    """The fold of the table's kind on the host: reply2_update_host for a ReplyTable2 (slots is then None) or a ReplyTables2."""
    if isinstance(replies, _PAIRS):
        return reply2_update_host(replies, recs, moves, won, records, playouts, slots)
    return reply_update_host(replies, recs, moves, won, records, playouts, slots)


def _update_device(recs, moves, won, records, playouts, replies, slots):
    """The same on the device, on the current stream: bkt_reply2_update(_tables) for a ReplyTable2 or a ReplyTables2, else
    bkt_reply_update(_tables)."""
    if isinstance(replies, _PAIRS):
        return T.reply2_update(recs, moves, won, records, playouts, replies.device(recs.device), slots=slots)
    return T.reply_update(recs, moves, won, records, playouts, replies.device(recs.device), slots=slots)


def _update_move_values_host(move_values, recs, moves, won, records, playouts, slots=None):
    """The update of the table's kind on the host: move_context_update_host for a MoveContextTable (no slots), else
    move_value_update_host."""
    if isinstance(move_values, MoveContextTable):
        return move_context_update_host(move_values, recs, moves, won, records, playouts)
    return move_value_update_host(move_values, recs, moves, won, records, playouts, _value_slots(move_values, slots))


def _update_move_values_device(recs, moves, won, records, playouts, move_values, slots=None):
    """bkt_move_value_update on the current stream: the table's tensors on the device of recs are the table from here on.
    With a MoveValueTables, bkt_move_value_update_tables with slots int32 [records] on the device; with a MoveContextTable,
    bkt_move_context_update."""
    counts, values, lut = move_values.device(recs.device)
    if isinstance(move_values, MoveContextTable):
        return T.move_context_update(recs, moves, won, records, playouts, counts, values, lut, move_values.k, move_values.limit,
                                     move_values.min_plays)
    return T.move_value_update(recs, moves, won, records, playouts, counts, values, lut, move_values.k, move_values.limit,
                               slots=_value_slots(move_values, slots))


def _value_slots(move_values, slots):
    """slots for the move-value calls: the checked slots with a MoveValueTables, None with a MoveValueTable."""
    return slots if isinstance(move_values, MoveValueTables) else None


def _check_tables(replies, move_values, slots, records):
    """replies=, move_values= and slots= of the callers here -> slots as an int64 array [records], or None without tables
    per game.  A MoveValueTables needs slots (TypeError), goes alone or with a ReplyTables or a ReplyTables2 of the same
    count (ValueError), and not with a single reply table (TypeError); everything else is _check_replies' and
    _check_move_values' rule."""
    if not isinstance(move_values, MoveValueTables):
        slots = _check_replies(replies, slots, records)
        _check_move_values(move_values, slots)
        return slots
    if slots is None:
        raise TypeError("move-value tables need slots: the table of every record")
    if replies is None:
        return slots_of(np.empty((1, 2, 81), np.uint8), _numpy(slots), records)
    if not isinstance(replies, (ReplyTables, ReplyTables2)):
        raise TypeError("a MoveValueTables keeps a table per game: with it replies= must be a ReplyTables or a ReplyTables2, "
                        "not a single table")
    if replies.count != move_values.count:
        raise ValueError(f"the reply tables and the move-value tables must be equally many (the same slots name both), "
                         f"got {replies.count} and {move_values.count}")
    return _check_replies(replies, slots, records)


def _check_move_values(move_values, slots):
    """move_values= of the callers here: None or a MoveValueTable, and never with slots= (there are no tables per game)."""
    if move_values is not None and not isinstance(move_values, MoveValueTable):
        raise TypeError("move_values must be a MoveValueTable or a MoveValueTables (it is updated in place) or None")
    if move_values is not None and slots is not None:
        raise TypeError("move_values= keeps one table for all records: not with slots= (a table per game)")


_PAIRS = (ReplyTable2, ReplyTables2)                                      # the tables keyed by the last two moves


def _check_replies(replies, slots=None, records=None):
    """replies= and slots= of the callers here -> slots as an int64 array [records], or None without tables (slots_of)."""
    if replies is not None and not isinstance(replies, ReplyTable):
        raise TypeError("replies must be a ReplyTable or a ReplyTables (it is updated in place) or None")
    return slots_of(replies, None if slots is None else _numpy(slots), records)


def _slots_device(slots, dev):
    """Checked slots as the launches take them: int32 on dev; None stays None."""
    return None if slots is None else torch.from_numpy(slots.astype(np.int32)).to(dev)


def _per_batch(call, *rows):
    """call(*chunks) for every T.MAX_BATCH rows of the tensors `rows` (a None among them is handed on as None), its results
    concatenated: a tensor, or a tuple of columns in which a None column stays None."""
    parts = [call(*(x if x is None else x[s:s + T.MAX_BATCH] for x in rows)) for s in range(0, len(rows[0]), T.MAX_BATCH)]
    if len(parts) == 1:
        return parts[0]
    if not isinstance(parts[0], tuple):
        return torch.cat(parts)
    return tuple(None if col[0] is None else torch.cat(col) for col in zip(*parts))


def _play_random_device(pos, key, ctr, max_plies, history, table=None, tactics=None, replies=None, slots=None, move_values=None):
    """pos uint8 [G,192] and ctr int32 [G,4] on the device; pos is played on in place; table: None or a PatternTable;
    tactics: None or a TacticTable; replies: None or a ReplyTable, which every launch reads as it stands, or a ReplyTables or
    a ReplyTables2 with slots int32 [G] on the device, the table of every row; move_values: None or a MoveValueTable, whose
    values every launch reads as they stand (bkt_move_value_playouts, with a ReplyTable or a ReplyTable2 put in; no slots),
    or a MoveValueTables with the same slots (bkt_move_value_playouts_tables, with a ReplyTables or a ReplyTables2 put in),
    or a MoveContextTable (bkt_move_context_playouts, with a ReplyTable or a ReplyTable2 put in; no slots).
    -> (over uint8 [G], plies int32 [G], moves int16 [G,max_plies] or None, status int32 [G]), T.MAX_BATCH rows per launch."""
    w, tac = (None if t is None else t.device(pos.device) for t in (table, tactics))
    if move_values is not None:
        put = {} if replies is None else {"replies2" if isinstance(replies, _PAIRS) else "replies": replies.device(pos.device)}
        values = move_values.device(pos.device)[1]
        if isinstance(move_values, MoveContextTable):                     # the table's class picks the kernel
            return _per_batch(lambda p, c: T.move_context_playouts(p, key, c, w, tac, values, max_plies, history=history, **put),
                              pos, ctr)
        return _per_batch(lambda p, c, s: T.move_value_playouts(p, key, c, w, tac, values, max_plies, history=history, slots=s,
                                                                **put), pos, ctr, _value_slots(move_values, slots))
    if replies is not None:
        play = T.reply2_playouts if isinstance(replies, _PAIRS) else T.reply_playouts
        tables = (w, tac, replies.device(pos.device))
    elif tactics is not None:
        play, tables = T.tactical_playouts, (w, tac)
    elif table is None:
        play, tables = T.random_playouts, ()
    else:
        play, tables = T.pattern_playouts, (w,)
    return _per_batch(lambda p, c, s: play(p, key, c, *tables, max_plies, history=history, **({} if s is None else {"slots": s})),
                      pos, ctr, slots)


def _area_score_device(pos, komi, owner):
    return _per_batch(lambda p: T.area_score(p, komi, owner=owner), pos)


def value_counters(recs, n):
    """The Philox counters of playout_value, int32 [R * n, 4] (numpy): playout j of a record whose Zobrist field is h uses
    (h & 0xFFFFFFFF, 0, h >> 32, 4 * j + STREAM_VALUE) -- the record names its own draws, never its row."""
    return L.game_counters(L.record_hash_words(recs).view(np.uint64), 0, L.value_streams(n))


def _check_playouts(n):
    n = int(n)
    if not 1 <= n < 2 ** 30:
        raise ValueError("the number of playouts must be at least 1 (and below 2^30)")
    return n


def _value_of_wins(w, n):
    """(2 w - n) / n as the host mirror's float32, on the device.  The device's float32 division is not correctly rounded
    (3 / 7 comes out one ulp high), its float64 division is; and rounding twice changes nothing below n = 2^29: a quotient
    of |x| <= 1 that is no float32 midpoint m lies at least |m| / (2^24 n) from it, beyond half a float64 ulp.  When n is a
    power of two both divisions are exact."""
    return ((2 * w - n).to(torch.float64) / n).to(torch.float32)


def _playouts(recs, n, key, rules, komi=L.KOMI, table=None, tactics=None, max_plies=MAX_PLIES, score=True, history=False,
              final=False, counted=0, sides=1, owned=0, replies=None, slots=None, move_values=None):
    """The one playout run: n playouts of each record of recs -- a uint8 [R,192] tensor on the device with
    rules="device", where nothing here waits for it; an array with "host", the mirror -- and what is asked of them, as a
    namespace whose fields are None when they were not asked for:
    value   float32 [R], wins [R]   (2 wins - n) / n; wins = the playouts the side to move at the record won
    won     bool [R,n]              which ones (score=True: from one bkt_area_score; score=False: no such launch, and wins
                                    comes from the owner counts of owned=True)
    moves   int16 [R * n, L]        history=True, or counted: the playout launch writes its history
    final   uint8 [R * n, 192]      final=True: the final records
    played, won_at                  counted=c (True: all): the AMAF counts of the first c records, int32 [c,81] from one
                                    bkt_amaf_counts, or with sides=2 [c,2,81] from one bkt_amaf_counts_sides
    owner                           owned=o (True: all): the five owner counts of the first o records, one bkt_owner_counts
    reply_plies                     replies= (a ReplyTable): every playout reads the table as it stands
                                    (bkt_reply_playouts, with history), and after the score one bkt_reply_update folds all
                                    R * n of them into it, in place and on the same stream; the plies the table decided on
                                    the host, None on the device, where nothing counts them.  It needs score=True: the
                                    update reads `won`.  With a ReplyTables, slots (an int array [R], required) is the
                                    table of every record, repeated per playout for the launch
                                    (bkt_reply_playouts_tables, bkt_reply_update_tables).  With a ReplyTable2
                                     the launches are bkt_reply2_playouts and bkt_reply2_update, slots is
                                    refused, and reply_pair_plies is the pair entries' share of reply_plies (host rules).
                                    With a ReplyTables2 slots is required again, and the launches are
                                    bkt_reply2_playouts_tables and bkt_reply2_update_tables.
    move_values=                    a MoveValueTable: every playout draws with its values as they stand
                                    (bkt_move_value_playouts, with history; replies= a ReplyTable or a ReplyTable2 composes),
                                    and after the score and the reply update one bkt_move_value_update folds all R * n of
                                    them into it, in place and on the same stream.  It needs score=True, and refuses slots.
                                    A MoveValueTables needs slots, the table of every record -- the same that
                                    name a ReplyTables' or a ReplyTables2's -- and the launches are
                                    bkt_move_value_playouts_tables and bkt_move_value_update_tables.  A MoveContextTable
                                     goes as a MoveValueTable does, on bkt_move_context_playouts and
                                    bkt_move_context_update."""
    R, host = len(recs), rules == "host"
    counted, owned = (R if x is True else int(x) for x in (counted, owned))
    slots = _check_tables(replies, move_values, slots, R)
    if replies is not None and not score:
        raise ValueError("a reply table learns from who won each playout: it needs the scored run (not playout_ownership's)")
    if move_values is not None and not score:
        raise ValueError("a move-value table learns from who won each playout: it needs the scored run (not playout_ownership's)")
    history = history or counted > 0 or replies is not None or move_values is not None
    if host:
        recs = np.array(_numpy(recs), np.uint8, order="C")
        fin = _random_host(np.repeat(recs, n, 0), key, value_counters(recs, n), max_plies, komi, history, table, tactics, replies,
                           None if slots is None else np.repeat(slots, n), move_values)
        pos, moves, black_wins = fin.records, fin.moves, fin.score.reshape(R, n) > 0
    else:
        pos = recs.repeat_interleave(n, 0)                                 # a copy: the caller's records stay
        slots = _slots_device(slots, recs.device)
        moves = _play_random_device(pos, key, L.value_counters_device(recs, n), max_plies, history, table, tactics, replies,
                                    None if slots is None else slots.repeat_interleave(n), move_values)[2]
        black_wins = _area_score_device(pos, komi, False).view(R, n) > 0 if score else None
    run = SimpleNamespace(value=None, wins=None, won=None, moves=moves, final=pos if final else None, played=None, won_at=None,
                          owner=None, reply_plies=None, reply_pair_plies=None)
    if score:
        run.won = black_wins == L.black_to_move(recs)[:, None]
        run.wins = run.won.sum(1)
    if replies is not None:                                                # playouts, then score, then update: submit order
        if host:
            run.reply_plies, run.reply_pair_plies = fin.reply_plies, fin.reply_pair_plies
            _update_host(replies, recs, moves, run.won.reshape(-1), R, n, slots)
        else:
            _update_device(recs, moves, run.won.reshape(-1).to(torch.uint8), R, n, replies, slots)
    if move_values is not None:                                            # ... then the move values, on the same stream
        if host:
            _update_move_values_host(move_values, recs, moves, run.won.reshape(-1), R, n, slots)
        else:
            _update_move_values_device(recs, moves, run.won.reshape(-1).to(torch.uint8), R, n, move_values, slots)
    if counted:
        reduce = ((T.amaf_counts, T.amaf_counts_sides), (amaf_counts_host, amaf_counts_sides_host))[host][sides - 1]
        won = run.won[:counted].reshape(-1)
        run.played, run.won_at = reduce(moves[:counted * n], won if host else won.to(torch.uint8), counted, n)
    if owned:
        run.owner = (owner_counts_host if host else T.owner_counts)(pos[:owned * n], owned, n, komi)
    if not score:
        bw = run.owner[4] if host else run.owner[4].to(torch.int64)
        run.wins = (np.where if host else torch.where)(L.black_to_move(recs), bw, n - bw)
    run.value = ((2 * run.wins - n).astype(np.float32) / np.float32(n)).astype(np.float32) if host else _value_of_wins(run.wins, n)
    return run


def _run(recs, n, seed, rules, komi, device, patterns, tactics, replies=None, slots=None, move_values=None, **ask):
    """What playout_value, playout_amaf and playout_ownership share: the checks, the upload and _playouts(**ask)."""
    L.check_rules(rules)
    table, tactics = _table(patterns), _tactics(tactics)
    n = _check_playouts(n)
    _check_records(recs)
    if rules == "device":
        recs = L.records_to_device(recs, _device(device, None, recs), clone=False)
    return _playouts(recs, n, L.seed_u64(seed), rules, komi, table, tactics, replies=replies, slots=slots,
                     move_values=move_values, **ask)


def playout_value(recs, n, seed, rules="device", komi=L.KOMI, device=None, patterns=None, tactics=None, replies=None,
                  slots=None, move_values=None):
    """The Monte-Carlo value of each record, float32 [R] (numpy): (2 w - n) / n, w = the number of n uniformly random
    eye-safe playouts (random_playouts, capped at MAX_PLIES and then scored as they stand) that the side to move wins --
    black wins iff the area score is > 0.  A pure function of the record, `seed` and `n` (value_counters): the row index
    and the rest of the batch do not enter.  recs: uint8 [R,192], numpy or a tensor.  patterns, tactics: as random_playouts.
    replies: None, or a ReplyTable the playouts read and this call then updates in place with all R * n of them:
    the value is then a function of the table as well.  slots: with a ReplyTables, the table of every record (random_playouts).
    move_values: None, or a MoveValueTable the playouts draw with and this call then updates in place."""
    return _numpy(_run(recs, n, seed, rules, komi, device, patterns, tactics, replies, slots, move_values).value)


class Amaf:
    """What playout_amaf returns, rows in the order of the records (numpy).

    value   float32 [R]     playout_value's value, bit for bit
    wins    int32 [R]       the playouts the side to move won: the w of (2 w - n) / n
    played  int32 [R,81]    the playouts in which the side to move was the first to play the point
    won     int32 [R,81]    those of them it won
    n       int             the playouts per record
    With playout_amaf(sides=2) played and won are [R,2,81]: [:, 0] as above, [:, 1] the same for the opponent, who wins
    the playouts the side to move loses (amaf_counts_sides_host has the definition).
    """

    def __init__(self, value, wins, played, won, n):
        self.value, self.wins, self.played, self.won, self.n = value, wins, played, won, int(n)


def _first_plies(moves, won, records, playouts):
    """The arguments of the two mirrors below, checked -> (first int64 [records * playouts, 81]: the smallest ply at which the
    row plays the point, P = max_plies: never; P; won as bool [records * playouts]; records; playouts)."""
    records, playouts = int(records), int(playouts)
    moves, won = np.asarray(moves), np.asarray(won).reshape(-1) != 0
    if records < 1 or playouts < 1 or moves.ndim != 2 or len(moves) != records * playouts or len(won) != len(moves):
        raise ValueError(f"moves must be [{records} * {playouts}, max_plies] and won [{records} * {playouts}]")
    G, P = moves.shape
    use = (np.cumsum(moves <= MOVE_NONE, 1) == 0) & (moves >= 0) & (moves <= 80)
    row, ply = np.nonzero(use)
    first = np.full((G, 81), P, np.int64)                                  # P: never played
    np.minimum.at(first, (row, moves[row, ply].astype(np.int64)), ply)
    return first, P, won, records, playouts


def amaf_counts_host(moves, won, records, playouts):
    """bkt_amaf_counts in numpy: moves int16 [records * playouts, max_plies] (a point 0..80, -1 = pass, <= MOVE_NONE ends the
    row, anything above 80 is ignored), won [records * playouts] (non-zero: the side to move at the record won the row's
    playout) -> (played, won_at) int32 [records, 81].  A row counts for the point s when the smallest ply k with
    moves[row, k] == s is even -- the side to move at the record plays the even plies: played += 1, won_at += the row's won."""
    first, P, won, records, playouts = _first_plies(moves, won, records, playouts)
    counts = (first < P) & (first % 2 == 0)
    played = counts.reshape(records, playouts, 81).sum(1)
    won_at = (counts & won[:, None]).reshape(records, playouts, 81).sum(1)
    return played.astype(np.int32), won_at.astype(np.int32)


def amaf_counts_sides_host(moves, won, records, playouts):
    """bkt_amaf_counts_sides in numpy (include/bokego_train.h has the definition): amaf_counts_host's moves and won ->
    (played, won_at) int32 [records, 2, 81].  A row counts for the point s and the side k & 1, k the smallest ply with
    moves[row, k] == s: side 0 is the side to move at the record and wins the rows with won != 0, side 1 its opponent, who
    wins the others.  [:, 0] is amaf_counts_host's result."""
    first, P, won, records, playouts = _first_plies(moves, won, records, playouts)
    played, won_at = np.zeros((2, records, 2, 81), np.int32)
    for side in (0, 1):
        counts = (first < P) & (first % 2 == side)
        played[:, side] = counts.reshape(records, playouts, 81).sum(1)
        won_at[:, side] = (counts & (won == (side == 0))[:, None]).reshape(records, playouts, 81).sum(1)
    return played, won_at


def playout_amaf(recs, n, seed, rules="device", komi=L.KOMI, device=None, patterns=None, tactics=None, sides=1, replies=None,
                 slots=None, move_values=None):
    """playout_value's n playouts of each record with what else they tell -> Amaf: the value (the history does not enter a
    game: the same bits), the wins, and the all-moves-as-first counts of every point (amaf_counts_host has the definition).
    rules="device": the playout launches with their history, `won` built in torch, one bkt_amaf_counts; rules="host": the
    mirror end to end, the same integers.  recs, patterns, tactics: as playout_value.
    sides=2: the counts of both sides, [R,2,81] (one bkt_amaf_counts_sides; amaf_counts_sides_host); value and wins are the
    same either way.  replies, slots, move_values: as playout_value."""
    if sides not in (1, 2):
        raise ValueError("sides must be 1 or 2")
    run = _run(recs, n, seed, rules, komi, device, patterns, tactics, replies, slots, move_values, counted=True, sides=sides)
    return Amaf(_numpy(run.value), _numpy(run.wins).astype(np.int32), _numpy(run.played), _numpy(run.won_at), n)


class Ownership:
    """What playout_ownership returns, rows in the order of the records (numpy).

    value       float32 [R]     playout_value's value, bit for bit
    wins        int32 [R]       the playouts the side to move won: black_wins for a record with black to move, else n - black_wins
    black       int32 [R,81]    the playouts at whose end the point was black's: a black stone or a black-only empty region
    white       int32 [R,81]    the same for white
    agree       int32 [R,81]    the playouts at whose end the point was the winner's
    hist        int32 [R,163]   the playouts by their margin before komi: bin d + 81, d = black's points - white's
    black_wins  int32 [R]       the playouts black won (area score > 0)
    n           int             the playouts per record
    mean_owner  float64 [R,81]  (black - white) / n: +1 black ... -1 white
    mean_margin float64 [R]     the mean of d
    """

    def __init__(self, value, wins, black, white, agree, hist, black_wins, n):
        self.value, self.wins, self.n = value, wins, int(n)
        self.black, self.white, self.agree, self.hist, self.black_wins = black, white, agree, hist, black_wins

    @property
    def mean_owner(self):
        return (self.black.astype(np.float64) - self.white.astype(np.float64)) / float(self.n)

    @property
    def mean_margin(self):
        return (self.hist.astype(np.float64) * np.arange(-81.0, 82.0)).sum(1) / float(self.n)

    def criticality(self):
        """Coulom's criticality of every point, float64 [R,81]: agree / n - (black / n * black_wins / n + white / n *
        (1 - black_wins / n)) -- how much more often the point goes to the winner than it would if owning it and winning
        were independent.  Computed here from the integers: device and host playouts give the same floats."""
        return criticality_of(self.black, self.white, self.agree, self.black_wins, self.n)


def criticality_of(black, white, agree, black_wins, n):
    """Ownership.criticality from the counts: [R,81] x3 and [R] integers, n playouts -> float64 [R,81]."""
    n = float(n)
    pb = (np.asarray(black_wins, np.float64) / n)[:, None]
    return np.asarray(agree, np.float64) / n - (np.asarray(black, np.float64) / n * pb
                                                + np.asarray(white, np.float64) / n * (1.0 - pb))


def owner_counts_host(final_recs, records, playouts, komi=L.KOMI):
    """bkt_owner_counts in numpy (include/bokego_train.h has the definition): final_recs uint8 [records * playouts, 192],
    the final records, rows r * playouts .. of record r -> (black, white, agree int32 [records, 81], hist int32
    [records, 163], black_wins int32 [records]).  The owner is owner_host's; a row is black's when
    (float32)B - ((float32)W + komi) > 0 in float32 arithmetic, bkt_area_score's expression."""
    records, playouts = int(records), int(playouts)
    recs = np.asarray(_numpy(final_recs))
    if records < 1 or playouts < 1 or recs.ndim != 2 or recs.shape != (records * playouts, POS_BYTES) or recs.dtype != np.uint8:
        raise ValueError(f"final_recs must be uint8 [{records} * {playouts}, {POS_BYTES}]")
    if not np.isfinite(np.float32(komi)):
        raise ValueError("komi must be finite")
    own = owner_host(recs)
    isb, isw = own > 0, own < 0
    B, W = isb.sum(1), isw.sum(1)
    bw = (B.astype(np.float32) - (W.astype(np.float32) + np.float32(komi))) > 0
    agree = (isb & bw[:, None]) | (isw & ~bw[:, None])
    black, white, agree = (x.reshape(records, playouts, 81).sum(1).astype(np.int32) for x in (isb, isw, agree))
    hist = np.zeros((records, 163), np.int32)
    np.add.at(hist, (np.repeat(np.arange(records), playouts), B - W + 81), 1)
    return black, white, agree, hist, bw.reshape(records, playouts).sum(1).astype(np.int32)


def playout_ownership(recs, n, seed, rules="device", komi=L.KOMI, device=None, patterns=None, tactics=None, replies=None,
                      move_values=None):
    """playout_value's n playouts of each record -- the same counters, draws and cap -- with what their final boards tell
    -> Ownership: the value (the same bits), the wins, and the ownership, agreement and margin counts of every record
    (owner_counts_host has the definition).  rules="device": the playout launch without history and one bkt_owner_counts;
    rules="host": the mirror end to end, the same integers.  recs, patterns, tactics: as playout_value.
    replies and move_values must be None: this run launches no score, and either table learns from who won (ValueError)."""
    run = _run(recs, n, seed, rules, komi, device, patterns, tactics, replies, move_values=move_values, score=False, owned=True)
    return Ownership(_numpy(run.value), _numpy(run.wins).astype(np.int32), *(_numpy(c) for c in run.owner), n)


PRIOR_K = 4.0              # amaf_prior's defaults: plausible, and not tuned
PRIOR_TEMPERATURE = 0.1


def legal_host(recs):
    """bool [n,81]: bk_pos_legal_moves of every record."""
    lib = go.golib()
    out = np.zeros((len(recs), 81), bool)
    buf = (ctypes.c_uint8 * 81)()
    for i in range(len(recs)):
        lib.bk_pos_legal_moves(L.pos_ptr(recs[i]), buf)
        out[i] = np.frombuffer(buf, np.uint8) != 0
    return out


def move_weights_host(recs, patterns=None, tactics=None):
    """bkt_move_weights in numpy (include/bokego_train.h has the definition): recs uint8 [R,192] (not modified); patterns,
    tactics: as random_playouts, None for none -> int32 [R,81]: tactics.combine of the pattern table's entries at
    patterns.codes_host and the tactics table's at tactics.codes_host on playable_host, 0 elsewhere."""
    from . import patterns as PT
    from . import tactics as TC
    table, tactics = _table(patterns), _tactics(tactics)
    recs = np.array(_numpy(recs), np.uint8, order="C")
    _check_records(recs)
    ok = playable_host(recs)
    entries = None if table is None else table.entries(PT.codes_host(recs))
    t = np.full(ok.shape, TC.NEUTRAL, np.uint16) if tactics is None else tactics.entries(TC.codes_host(recs))
    return np.where(ok, TC.combine(entries, t), 0).astype(np.int32)


def move_weights(recs, patterns=None, tactics=None, rules="device", device=None):
    """The weight the playouts' draw gives every point of every record at the first ply, 0 where the point is not playable
    -> int32 [R,81] (numpy).  rules="device": one bkt_move_weights launch per T.MAX_BATCH records; rules="host":
    move_weights_host, the same integers without a GPU.  recs, patterns, tactics: as playout_value."""
    L.check_rules(rules)
    if rules == "host":
        return move_weights_host(recs, patterns, tactics)
    table, tactics = _table(patterns), _tactics(tactics)
    _check_records(recs)
    t = L.records_to_device(recs, _device(device, None, recs), clone=False)
    return _move_weights_device(t, table, tactics).cpu().numpy()


def _move_weights_device(recs, table, tactics):
    """recs: a uint8 [R,192] tensor on the device -> int32 [R,81] on the device; nothing here waits for it."""
    tables = (None if table is None else table.device(recs.device), None if tactics is None else tactics.device(recs.device))
    return _per_batch(lambda r: T.move_weights(r, *tables), recs)


def _not_negative(x, name):
    x = float(x)
    if not 0.0 <= x < float("inf"):
        raise ValueError(f"{name} must be finite and not negative")
    return x


def _log_weights(weights, R):
    """ln max(w, 1) of move weights [R,81], float64: a point off the playable set enters with the least weight, 1."""
    w = np.asarray(_numpy(weights))
    if w.shape != (R, 81):
        raise ValueError(f"weights must be [{R}, 81], one row per record")
    return np.log(np.maximum(w.astype(np.float64), 1.0))


def _over_legal(recs, x, shifted):
    """What the priors below share: p = exp(shifted(top)) on the legal points (bk_pos_legal_moves), top = the maximum of x
    [R,81] over them, 0 elsewhere, each row divided by its sum -> float32 [R,81]; 1/81 everywhere in a row without a legal
    point.  The argument of exp stays with the caller: the three of them round differently."""
    legal = legal_host(recs)
    some = legal.any(1)
    top = np.where(legal, x, -np.inf).max(1, keepdims=True)
    top[~some] = 0.0
    p = np.where(legal, np.exp(shifted(top)), 0.0)
    p[~some] = 1.0
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def pattern_prior(recs, weights, mu=1.0):
    """The move predictor's own prediction -> float32 [R,81], in float64 on the host: with weights = move_weights(recs, ...),
    p_s = exp(mu * (ln max(w_s, 1) - the maximum over the legal points)) on the legal points (bk_pos_legal_moves), 0
    elsewhere, each row divided by its sum; a record without a legal point gets 1/81 everywhere.  mu = 1: in proportion to
    the weights.  mu must be finite and not negative."""
    mu = _not_negative(mu, "mu")
    recs = np.array(_numpy(recs), np.uint8, order="C")
    _check_records(recs)
    lw = _log_weights(weights, len(recs))
    return _over_legal(recs, lw, lambda top: mu * (lw - top))


def amaf_prior(recs, amaf, k=PRIOR_K, temperature=PRIOR_TEMPERATURE, criticality=None, gamma=0.0, weights=None, mu=0.0):
    """A search prior from the counts of playout_amaf(recs, ...) -> float32 [R,81], computed on the host in float64 from the
    integers, so that device and host playouts give the same floats.  With wbar = wins / n, the win rate of all n playouts,
        q_s = (won_s + k * wbar) / (played_s + k)      the AMAF win rate of the point, k playouts' worth of wbar mixed in,
        p_s = exp((q_s - max q over the legal points) / temperature) on the legal points (bk_pos_legal_moves), 0 elsewhere,
    each row divided by its sum; a record without a legal point gets 1/81 everywhere.  k and temperature must be > 0; their
    defaults, 4.0 and 0.1, are plausible and untuned.  Two-sided counts ([R,2,81], playout_amaf(sides=2)) are read at side 0.
    criticality (float64 [R,81], Ownership.criticality()) with gamma > 0: q_s + gamma * criticality_s takes the place of q_s
    (gamma is untuned).  criticality=None or gamma == 0: the floats above, bit for bit.  gamma must be finite and
    not negative.
    weights (int [R,81], move_weights(recs, ...)) with mu > 0: the logit of a legal point is
    (q_s + gamma * criticality_s) / temperature + mu * ln(max(w_s, 1)), shifted by its maximum over the legal points before
    exp (mu is untuned); a legal point off the playable set (an own eye) enters with the least weight, 1.
    weights=None or mu == 0: the floats above, bit for bit.  mu must be finite and not negative."""
    k, temperature, mu = float(k), float(temperature), _not_negative(mu, "mu")
    if not k > 0 or not temperature > 0:
        raise ValueError("k and temperature must be greater than 0")
    gamma = _not_negative(gamma, "gamma")
    recs = np.array(_numpy(recs), np.uint8, order="C")
    _check_records(recs)
    played, won = np.asarray(amaf.played, np.float64), np.asarray(amaf.won, np.float64)
    if played.shape == (len(recs), 2, 81) and won.shape == played.shape:   # two-sided counts: the side to move's half
        played, won = played[:, 0], won[:, 0]
    if played.shape != (len(recs), 81) or won.shape != played.shape:
        raise ValueError(f"the counts must be [{len(recs)}, 81] or [{len(recs)}, 2, 81], one row per record")
    wbar = np.asarray(amaf.wins, np.float64) / float(amaf.n)
    q = (won + k * wbar[:, None]) / (played + k)
    if criticality is not None and gamma > 0.0:
        crit = np.asarray(criticality, np.float64)
        if crit.shape != q.shape:
            raise ValueError(f"criticality must be [{len(recs)}, 81], one row per record")
        q = q + gamma * crit
    if weights is not None and mu > 0.0:
        z = q / temperature + mu * _log_weights(weights, len(recs))
        return _over_legal(recs, z, lambda top: z - top)
    return _over_legal(recs, q, lambda top: (q - top) / temperature)


class PlayoutEvaluator:
    """A tree-search evaluator (NativeMCTS(evaluator=), selfplay.self_play, the GTP front-end) without a value net: the
    priors of a request's first n_policy rows come from `engine` (a LeafEngine with policy weights, asked as
    selfplay.EngineEvaluator(value=False) asks), the values of all its rows from playout_value(playouts, seed).  The
    engine's request and the playout launch do not depend on each other and are in flight together between submit and
    finish.  rules="host": the values from the host mirror (the same bits; for tests).
    prior (0..1, default 0: exactly the above) mixes the priors with what the request's own playouts say about the moves:
    the playouts then run with their history (playout_amaf), the counts of the first n_policy rows give amaf_prior(k=prior_k,
    temperature=prior_temperature), and the priors handed on are (1 - prior) * the engine's + prior * amaf_prior, mixed in
    float64, cast to float32 and normalised as before.  With prior=1 the engine is never asked and may be None: a search
    without any network.
    rave=True: the playouts of ALL rows run with their history, one bkt_amaf_counts_sides reduces them, and finish returns a
    third element, records = (playouts, wins int32 [B], played int32 [B,2,81], won_at int32 [B,2,81]), which
    selfplay.GamePool.deliver hands to the tree's RAVE tables; the prior, when prior > 0, reads side 0 of the first
    n_policy rows of the same counts -- one reduction launch, not two.  Probs and values are what they are without it.
    criticality (gamma >= 0, default 0: exactly the above, the same launches; it needs prior > 0): the playouts keep their
    final records, one bkt_owner_counts over the first n_policy rows gives their Ownership counts, and amaf_prior gets
    criticality = Coulom's criticality of every point and gamma (untuned).  The values of all rows and, with
    rave=True, the records are what they are without it.
    pattern_prior (mu >= 0, default 0: exactly the above, the same launches; it needs prior > 0): one bkt_move_weights over
    the first n_policy rows (the host mirror with rules="host") gives their move weights, and amaf_prior gets them and mu
    (untuned).  The tables of that term are prior_patterns and prior_tactics, which default to the playouts' own
    patterns and tactics -- so uniform playouts can run under a pattern prior; with no table at all every weight would be
    equal: ValueError.  Values and records are what they are without it.
    replies=True (default False: exactly the above, the same launches): the evaluator owns one ReplyTable, created empty,
    `.replies`, which reset_replies() clears.  The playouts of every request read it (bkt_reply_playouts: the last good reply
    to the move before, where it is playable, instead of the draw) and are folded into it after their score (one
    bkt_reply_update), all on one stream: playouts, then score, then update, so two requests in flight see the table in
    submit order.  Values, priors, RAVE records and criticality are computed as before from that run.  With replies=True a
    value is no longer a function of (record, seed, N) alone: it is a function of those and the requests submitted before
    it.  A given tree search is still deterministic per seed, and device rules and host rules give the same bits.
    games=G (with replies=True; default None: the one table above, the same launches): `.replies` is a ReplyTables(G), a table
    per game of a self-play batch, and submit takes games=, the table of every row (selfplay.run_pools passes them); one
    bkt_reply_playouts_tables and one bkt_reply_update_tables serve all games of a request.  `wants_games` says
    which of the two an instance is.
    replies=2: `.replies` is a ReplyTable2, replies keyed by the last two moves with the single-move table as its
    plane 81 (bkt_reply2_playouts, bkt_reply2_update; the same stream order, the same determinism).  replies=2 with games= is
    a TypeError: pair tables per game are the next keyword.
    pair_games=G (default None: exactly the above; without replies= and games=, TypeError with either): `.replies` is a
    ReplyTables2(G), a pair table per game, and submit takes games= as with games=G; one bkt_reply2_playouts_tables and one
    bkt_reply2_update_tables serve all games of a request.  A one-game pool is then replies=2 bit for bit.
    move_values=True or a temperature tau > 0 (default False: exactly the above, the same launches): the evaluator
    owns one movevalues.MoveValueTable, created empty (tau; True: DEFAULT_TAU; k and limit the module's defaults),
    `.move_values`, which reset_move_values() clears.  The playouts of every request draw with its values
    (bkt_move_value_playouts, composed with replies=True or replies=2) and are folded into it after their score and the
    reply update (bkt_move_value_update), all on the one stream.  A fresh table is neutral: the first request equals the
    evaluator without the option bit for bit.  With games= or pair_games= it is a TypeError: that is move_value_games=.
    move_value_games=G (default None: exactly the above): `.move_values` is a movevalues.MoveValueTables(G,
    tau=move_value_tau), a move-value table per game, wants_games is true and submit takes games=, the table of every row;
    one bkt_move_value_playouts_tables and one bkt_move_value_update_tables serve all games of a request.  It goes alone,
    with replies=True, games=G or with pair_games=G -- the same G (ValueError), the same games= naming both tables of a row
    -- and not with move_values=, nor with replies=True or replies=2 without tables per game (TypeError).  A one-game pool
    is then move_values=tau bit for bit.
    move_contexts=True or a temperature tau > 0 (default False: exactly the above): `.move_values` is a
    movecontexts.MoveContextTable, created empty (tau; True: DEFAULT_TAU; k, limit and min_plays the modules' defaults),
    which reset_move_values() clears: the playouts of every request draw with its values (bkt_move_context_playouts,
    composed with replies=True or replies=2) and are folded into it (bkt_move_context_update) where move_values= has its
    two calls.  Not with move_values= (the table contains that one as its plane 81), games=, pair_games= or
    move_value_games= (TypeError): a context table per game is not built.
    The engine is kept as `policy_engine`, not `engine`: selfplay.run_pools_native hands an evaluator's `engine` to the C
    step loop as its own bk_evaluator, which would compute no playouts -- this class goes through callback_evaluator."""
    wants_positions = True
    wants_games = False                                                   # True: submit needs games=, a table per game

    def __init__(self, engine, playouts=64, seed=0, rules="device", komi=L.KOMI, patterns=None, tactics=None, prior=0.0,
                 prior_k=PRIOR_K, prior_temperature=PRIOR_TEMPERATURE, rave=False, criticality=0.0, pattern_prior=0.0,
                 prior_patterns=None, prior_tactics=None, move_values=False, move_value_games=None, move_value_tau=DEFAULT_TAU,
                 move_contexts=False, replies=False, games=None, pair_games=None):
        L.check_rules(rules)
        if move_contexts and (move_values or games is not None or pair_games is not None or move_value_games is not None):
            raise TypeError("move_contexts= keeps one move-context table for all rows, whose plane 81 is the move-value table: "
                            "it goes without move_values=, games=, pair_games= and move_value_games=")
        if move_values and (games is not None or pair_games is not None):
            raise TypeError("move_values= keeps one table for all rows: it goes without games= and pair_games= (a table per game)")
        # True: the default temperature; a number: tau; False, None or 0: no table
        self.move_values = (MoveValueTable.empty() if move_values is True else MoveValueTable.empty(tau=move_values)) \
            if move_values else None
        if move_contexts:
            self.move_values = MoveContextTable.empty() if move_contexts is True else MoveContextTable.empty(tau=move_contexts)
        if move_value_games is not None:
            if move_values:
                raise TypeError("move_value_games= is the number of move-value tables, a MoveValueTables: it goes without "
                                "move_values= (one table for all rows)")
            if replies and games is None:
                raise TypeError("move_value_games= keeps a table per game: with it the reply tables are per game too "
                                "(replies=True, games=G, or pair_games=G), not one for all rows")
            for other in (games, pair_games):
                if other is not None and int(other) != int(move_value_games):
                    raise ValueError(f"the reply tables and the move-value tables must be equally many (games= names both "
                                     f"tables of a row), got {other} and {move_value_games}")
            self.move_values = MoveValueTables(move_value_games, tau=move_value_tau)
        if pair_games is not None and (replies or games is not None):
            raise TypeError("pair_games= is the number of pair reply tables, a ReplyTables2: it goes without replies= and games=")
        if games is not None and not replies:
            raise TypeError("games= is the number of reply tables: it needs replies=True")
        if replies == 2 and not isinstance(replies, bool):
            if games is not None:
                raise TypeError("replies=2 goes without games= (replies=True takes it): pair reply tables per game are pair_games=G")
            self.replies = ReplyTable2.empty()
        elif pair_games is not None:
            self.replies = ReplyTables2(pair_games)
        else:
            self.replies = (ReplyTable.empty() if games is None else ReplyTables(games)) if replies else None
        if games is not None or pair_games is not None or move_value_games is not None:
            self.wants_games = True
        self.rave = bool(rave)
        self.criticality = _not_negative(criticality, "criticality")
        if self.criticality > 0.0 and not float(prior) > 0.0:
            raise ValueError("criticality is a term of the playout prior: it needs prior > 0")
        self.patterns = _table(patterns)                                  # None: uniformly random playouts
        self.tactics = _tactics(tactics)                                  # None: no tactical weights
        self.pattern_prior = _not_negative(pattern_prior, "pattern_prior")
        if self.pattern_prior > 0.0 and not float(prior) > 0.0:
            raise ValueError("pattern_prior is a term of the playout prior: it needs prior > 0")
        self.prior_patterns = self.patterns if prior_patterns is None else _table(prior_patterns)
        self.prior_tactics = self.tactics if prior_tactics is None else _tactics(prior_tactics)
        if self.pattern_prior > 0.0 and self.prior_patterns is None and self.prior_tactics is None:
            raise ValueError("pattern_prior needs a table: patterns, tactics, prior_patterns or prior_tactics")
        self.prior = float(prior)
        if not 0.0 <= self.prior <= 1.0:
            raise ValueError("prior must be within 0..1")
        self.prior_k, self.prior_temperature = float(prior_k), float(prior_temperature)
        if not self.prior_k > 0 or not self.prior_temperature > 0:
            raise ValueError("prior_k and prior_temperature must be greater than 0")
        if engine is None and self.prior < 1.0:
            raise TypeError("engine=None goes with prior=1.0 only: below it the priors need a policy engine")
        self.policy_engine = engine
        self.playouts = _check_playouts(playouts)
        self.seed = L.seed_u64(seed)
        self.rules, self.komi = rules, komi
        self.positions = self.batches = 0

    def submit(self, recs, n_policy, games=None):
        recs = np.ascontiguousarray(recs, np.uint8)
        if recs.ndim != 2 or recs.shape[1] != POS_BYTES:
            raise ValueError(f"a PlayoutEvaluator takes position records uint8 [B, {POS_BYTES}], got {recs.shape}")
        if self.wants_games and games is None:
            raise TypeError("this evaluator keeps a table per game: submit needs games=, the table of every row")
        if not self.wants_games and games is not None:
            raise TypeError("games= names the tables of the rows: this evaluator keeps none per game (replies=True, games=G, "
                            "pair_games=G or move_value_games=G)")
        self.positions += len(recs)
        self.batches += 1
        ticket = None
        if n_policy and self.prior < 1.0:
            ticket = self.policy_engine.submit_positions(recs[:n_policy], logits=False, probs=True, value=False,
                                                         n_policy=n_policy)
        counted = n_policy if n_policy and self.prior > 0.0 else 0        # the rows whose prior the playouts have a share in
        weights, host = None, self.rules == "host"
        t = recs if host else torch.from_numpy(recs).to(_device(None, self.policy_engine))
        # rave: every row with its history, both sides counted, and the prior reads side 0 of the first rows of those counts
        run = _playouts(t, self.playouts, self.seed, self.rules, self.komi, self.patterns, self.tactics,
                        counted=len(recs) if self.rave else counted, sides=2 if self.rave else 1,
                        owned=counted if self.criticality > 0.0 else 0, replies=self.replies, slots=games,
                        move_values=self.move_values)
        if counted and self.pattern_prior > 0.0:                          # (the device's launch: nothing waits for it)
            weights = (move_weights_host if host else _move_weights_device)(t[:counted], self.prior_patterns, self.prior_tactics)
        return SimpleNamespace(ticket=ticket, run=run, n_policy=counted, weights=weights, recs=recs[:counted])

    def reset_replies(self):
        """An empty reply table again (replies=True; every table with games=G or pair_games=G): what a new game starts with."""
        if self.replies is None:
            raise TypeError("this evaluator keeps no reply table: replies=True")
        self.replies.clear()

    def reset_move_values(self):
        """An empty move-value table again (move_values=True or tau; every table with move_value_games=G): what a new game
        starts with."""
        if self.move_values is None:
            raise TypeError("this evaluator keeps no move-value table: move_values=True, move_contexts=True or move_value_games=G")
        self.move_values.clear()

    def finish(self, handle, normalise=None):
        run, n = handle.run, handle.n_policy
        if normalise is None:
            from .selfplay import normalise_like_categorical as normalise
        probs = np.zeros((0, 81), np.float32) if handle.ticket is None else self.policy_engine.wait(handle.ticket)["probs"]
        records = None
        if self.rave or n:
            w, played, won = (_numpy(x) for x in (run.wins, run.played, run.won_at))
        if self.rave:                                                     # (w, played, won_at) of every row, two-sided
            w, played, won = (np.ascontiguousarray(x, np.int32) for x in (w, played, won))
            records = (self.playouts, w, played, won)
        if n:
            crit = None
            if run.owner is not None:
                black, white, agree, _, black_wins = (_numpy(x) for x in run.owner)
                crit = criticality_of(black, white, agree, black_wins, self.playouts)
            prior = amaf_prior(handle.recs, Amaf(None, w[:n], played[:n], won[:n], self.playouts), self.prior_k,
                               self.prior_temperature, criticality=crit, gamma=self.criticality, weights=_numpy(handle.weights),
                               mu=self.pattern_prior)
            if handle.ticket is not None:
                prior = ((1.0 - self.prior) * probs.astype(np.float64) + self.prior * prior.astype(np.float64))
            probs = prior.astype(np.float32)
        if len(probs):
            probs = normalise(probs)
        return (probs, _numpy(run.value), records) if records is not None else (probs, _numpy(run.value))

    def __call__(self, recs, n_policy):
        return self.finish(self.submit(recs, n_policy))


# ---- the Monte-Carlo score ------------------------------------------------------------------------------------------------
class RolloutScore:
    """rollout_score's result for one position.

    mean_owner  float64 [81]   mean of the final owner over the n playouts (+1 black ... -1 white)
    black_win   float          share of playouts black won (final area score > 0)
    mean_score  float          mean final area score
    score       float          area by majority ownership: (points with mean > 0) - ((points with mean < 0) + komi)
    status      list [81]      None for an empty point, else "alive", "dead" or "seki"
    """

    def stones(self, status):
        return [s for s in range(81) if self.status[s] == status]


def _as_records(positions):
    if isinstance(positions, np.ndarray) and positions.dtype == np.uint8:
        recs = positions.reshape(-1, POS_BYTES)
    else:
        if isinstance(positions, go.Game):
            positions = [positions]
        recs = np.stack([np.frombuffer(bytes(g._pos), np.uint8) for g in positions])
    return np.ascontiguousarray(recs)


def rollout_score(positions, engine, n=256, seed=0, komi=L.KOMI, rules="device", max_plies=MAX_PLIES, device=None,
                  one_launch=False, patterns=None, tactics=None):
    """n playouts (finish_games) of every position -> a list of RolloutScore.  positions: go.Game objects or uint8
    [P,192] records.  Playout j of position i is game i * n + j of one finish_games call: deterministic per seed.
    one_launch=True (engine must be None): the uniformly random playouts of random_playouts instead, any number of rows;
    patterns, tactics (with one_launch=True only): random_playouts' tables of pattern and of tactical weights."""
    recs = _as_records(positions)
    n = _check_playouts(n)
    P = len(recs)
    if patterns is not None and not one_launch:
        raise ValueError("patterns weight the one-launch playouts: one_launch=True")
    if tactics is not None and not one_launch:
        raise ValueError("tactics weight the one-launch playouts: one_launch=True")
    if one_launch:
        if engine is not None:
            raise ValueError("one_launch=True plays uniformly random playouts: engine must be None")
        fin = random_playouts(np.repeat(recs, n, 0), seed, max_plies=max_plies, rules=rules, komi=komi, history=False,
                              device=device, patterns=patterns, tactics=tactics)
    else:
        fin = finish_games(np.repeat(recs, n, 0), engine, seed, max_plies=max_plies, rules=rules, device=device, komi=komi)
    owner = fin.owner.reshape(P, n, 81).astype(np.float64).mean(1)
    score = fin.score.reshape(P, n).astype(np.float64)
    out = []
    for i in range(P):
        r = _score_of_owner(recs[i], owner[i], float((score[i] > 0).mean()), float(score[i].mean()), komi)
        r.unfinished = int((~fin.over.reshape(P, n)[i]).sum())
        out.append(r)
    return out


def _score_of_owner(rec, mean_owner, black_win, mean_score, komi):
    """A RolloutScore (without `unfinished`) from a record's mean ownership: the area by majority ownership and the status of
    every stone, seki where |mean ownership| is below SEKI_THRESHOLD."""
    r = RolloutScore()
    r.mean_owner, r.black_win, r.mean_score = mean_owner, black_win, mean_score
    r.score = float((mean_owner > 0).sum()) - (float((mean_owner < 0).sum()) + float(komi))
    board = rec[:81].view(np.int8)
    r.status = [None] * 81
    for s in np.nonzero(board)[0].tolist():
        sign = 1.0 if board[s] == 1 else -1.0
        m = mean_owner[s]
        r.status[s] = "seki" if abs(m) < SEKI_THRESHOLD else ("alive" if m * sign > 0 else "dead")
    return r


def ownership_score(positions, n, seed, komi=L.KOMI, **kw):
    """rollout_score's score and status rules on playout_ownership's counts -> a list of RolloutScore (mean_score: the mean
    margin less komi; no `unfinished`).  positions: go.Game objects or uint8 [P,192] records; kw: playout_ownership's rules,
    device, patterns and tactics.  No network and no owner array: what the net-free GTP engine scores its games with."""
    recs = _as_records(positions)
    o = playout_ownership(recs, n, seed, komi=komi, **kw)
    owner, margin = o.mean_owner, o.mean_margin
    return [_score_of_owner(recs[i], owner[i], float(o.black_wins[i]) / o.n, float(margin[i]) - float(komi), komi)
            for i in range(len(recs))]


def format_score(score):
    """GTP's final_score answer: B+3.5, W+2.5 or 0."""
    return "0" if score == 0 else f"{'B' if score > 0 else 'W'}+{abs(score):g}"


def owner_board(mean_owner):
    """Nine lines: X / O where the mean ownership is beyond +-SEKI_THRESHOLD, x / o for a weaker lean, . for none."""
    rows = []
    for r in range(9):
        cells = []
        for c in range(9):
            m = mean_owner[9 * r + c]
            cells.append("X" if m >= SEKI_THRESHOLD else "O" if m <= -SEKI_THRESHOLD else "x" if m > 0 else
                         "o" if m < 0 else ".")
        rows.append(" ".join(cells))
    return "\n".join(rows)


# ---- the command line --------------------------------------------------------------------------------------------------------
def _parse(argv):
    ap = argparse.ArgumentParser(description="Score a position of an SGF by policy playouts to the end of the game")
    ap.add_argument("--sgf", required=True, help="the game record")
    ap.add_argument("--move", type=int, default=None, help="score the position after K moves (default: the last)")
    ap.add_argument("-p", dest="p", metavar="POLICY", default=None,
                    help="policy weights (.pt or .bkw); without it the playouts are uniformly random")
    ap.add_argument("--random", action="store_true",
                    help="uniformly random playouts, each played to its end inside one kernel launch (not with -p)")
    ap.add_argument("--patterns", default=None, metavar="FILE",
                    help="with --random: draw the moves by the 3x3 pattern weights of this table (python -m bokego_amd.patterns fit)")
    ap.add_argument("--tactics", default=None, metavar="FILE",
                    help="with --random: multiply the weights by the tactical weights of this table (python -m bokego_amd.tactics fit)")
    ap.add_argument("--amaf", action="store_true",
                    help="with --random: print the Monte-Carlo value and the ten heaviest moves of the AMAF prior instead of the score")
    ap.add_argument("--ownership", action="store_true",
                    help="with --random: print the ownership map, the mean margin and the ten most critical points instead of the score")
    ap.add_argument("--weights", action="store_true",
                    help="with --random: print the ten heaviest points of the position by the playouts' move weights "
                         "(--patterns, --tactics) instead of the score; no playout runs")
    ap.add_argument("--replies", action="store_true",
                    help="with --random: play the playouts in chunks that learn a last-good-reply table from each other, and "
                         "print the share of plies the table decided and its occupancy instead of the score")
    ap.add_argument("--reply-pairs", action="store_true",
                    help="with --random: as --replies with a table keyed by the last two moves (LGRF-2): print the shares of "
                         "plies its pair entries and its single entries decided, and the occupancy of both parts")
    ap.add_argument("--move-values", action="store_true",
                    help="with --random: play the playouts in chunks that learn a move-value table from each other (MAST), and "
                         "print the share of its entries that were played, its smallest and largest value and its ten "
                         "heaviest points instead of the score")
    ap.add_argument("--move-contexts", action="store_true",
                    help="with --random: as --move-values with a table keyed by the previous move as well (NAST): print also "
                         "the share of its context entries that have their minimum of plays")
    ap.add_argument("--chunk", type=int, default=16, metavar="C",
                    help="with --replies, --reply-pairs, --move-values or --move-contexts: playouts per chunk")
    ap.add_argument("--sides", type=int, default=1, choices=(1, 2),
                    help="with --amaf: 2 also prints the opponent's heaviest points (the two-sided counts RAVE is fed with)")
    ap.add_argument("-n", dest="n", type=int, default=256, help="playouts")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--komi", type=float, default=L.KOMI)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.amaf and not args.random:
        ap.error("--amaf reads the one-launch playouts: it needs --random")
    if args.ownership and (not args.random or args.amaf):
        ap.error("--ownership reads the one-launch playouts: it needs --random, and not --amaf")
    if args.weights and (not args.random or args.amaf or args.ownership):
        ap.error("--weights reads the one-launch playouts' draw: it needs --random, and not --amaf or --ownership")
    if args.replies and (not args.random or args.amaf or args.ownership or args.weights):
        ap.error("--replies reads the one-launch playouts: it needs --random, and not --amaf, --ownership or --weights")
    if args.reply_pairs and (not args.random or args.amaf or args.ownership or args.weights or args.replies):
        ap.error("--reply-pairs reads the one-launch playouts: it needs --random, and not --amaf, --ownership, --weights or "
                 "--replies (pairs contain singles)")
    if args.move_values and (not args.random or args.amaf or args.ownership or args.weights or args.replies or args.reply_pairs):
        ap.error("--move-values reads the one-launch playouts: it needs --random, and not --amaf, --ownership, --weights, "
                 "--replies or --reply-pairs")
    if args.move_contexts and (not args.random or args.amaf or args.ownership or args.weights or args.replies
                               or args.reply_pairs or args.move_values):
        ap.error("--move-contexts reads the one-launch playouts: it needs --random, and not --amaf, --ownership, --weights, "
                 "--replies, --reply-pairs or --move-values (contexts contain the plain values)")
    if args.chunk < 1:
        ap.error("--chunk must be at least 1")
    if args.sides != 1 and not args.amaf:
        ap.error("--sides goes with --amaf")
    if args.n < 1:
        ap.error("-n must be at least 1")
    if args.random and args.p is not None:
        ap.error("--random plays without a network: not with -p")
    if args.patterns is not None and not args.random:
        ap.error("--patterns weights the one-launch playouts: it needs --random")
    if args.tactics is not None and not args.random:
        ap.error("--tactics weights the one-launch playouts: it needs --random")
    if args.move is not None and args.move < 0:
        ap.error("--move must not be negative")
    if not (0 <= args.seed < 2 ** 64):
        ap.error("--seed must be an unsigned 64-bit integer")
    return args


def sgf_position(path, move=None):
    """The position after `move` moves of the SGF (all of them by default)."""
    moves = go.get_moves(path)
    g = go.Game()
    for mv in moves[:len(moves) if move is None else move]:
        if mv == go.PASS:
            g.play_pass()
        else:
            g.play_move(mv)
    return g


def reply_report(recs, n, seed, chunk, rules="device", komi=L.KOMI, **kw):
    """n playouts of the one record recs [1,192] in chunks of `chunk`, each chunk reading the reply table the chunks before
    it left (random_playouts(replies=); game g of the n keeps default_counters' words, so the chunking changes the table a
    game sees and nothing else) -> a dict: the plies played, those the table decided, their share, the table's occupancy
    at the end and black's share of the wins.  kw: random_playouts' patterns, tactics and device."""
    table, plies, decided, black = ReplyTable.empty(), 0, 0, 0
    ctr = default_counters(n, np.repeat(record_turns(recs), n))
    for s in range(0, n, chunk):
        c = min(chunk, n - s)
        before = table.copy()
        fin = random_playouts(np.repeat(recs, c, 0), seed, counters=ctr[s:s + c], rules=rules, komi=komi, replies=table, **kw)
        plies += int(fin.plies.sum())
        decided += reply_plies_of(before, np.repeat(recs, c, 0), fin.moves, 1)
        black += int((fin.score > 0).sum())
    return {"playouts": n, "chunk": chunk, "plies": plies, "reply_plies": decided, "share": decided / max(plies, 1),
            "occupancy": table.occupancy(), "black_win": black / n}


def reply_pairs_report(recs, n, seed, chunk, rules="device", komi=L.KOMI, **kw):
    """reply_report with a ReplyTable2 -> a dict: the plies played, those the pair entries and the single
    entries decided and their shares, the occupancy of both parts of the table at the end and black's share of the wins."""
    table, plies, pair, single, black = ReplyTable2.empty(), 0, 0, 0, 0
    ctr = default_counters(n, np.repeat(record_turns(recs), n))
    for s in range(0, n, chunk):
        c = min(chunk, n - s)
        before = table.copy()
        fin = random_playouts(np.repeat(recs, c, 0), seed, counters=ctr[s:s + c], rules=rules, komi=komi, replies=table, **kw)
        plies += int(fin.plies.sum())
        by_pair, by_single = reply2_plies_of(before, np.repeat(recs, c, 0), fin.moves, 1)
        pair, single = pair + by_pair, single + by_single
        black += int((fin.score > 0).sum())
    return {"playouts": n, "chunk": chunk, "plies": plies, "pair_plies": pair, "single_plies": single,
            "pair_share": pair / max(plies, 1), "single_share": single / max(plies, 1),
            "pair_occupancy": table.pairs_occupancy(), "single_occupancy": table.singles().occupancy(), "black_win": black / n}


def move_values_report(recs, n, seed, chunk, rules="device", komi=L.KOMI, **kw):
    """reply_report with a MoveValueTable of the default parameters -> a dict: the plies played, the share of
    the table's 162 entries with a play, its smallest and largest value, the ten heaviest entries and black's share of the
    wins."""
    table, plies, black = MoveValueTable.empty(), 0, 0
    ctr = default_counters(n, np.repeat(record_turns(recs), n))
    for s in range(0, n, chunk):
        c = min(chunk, n - s)
        fin = random_playouts(np.repeat(recs, c, 0), seed, counters=ctr[s:s + c], rules=rules, komi=komi, move_values=table, **kw)
        plies += int(fin.plies.sum())
        black += int((fin.score > 0).sum())
    values, counts = table.values.reshape(-1), table.counts.reshape(162, 2)
    return {"playouts": n, "chunk": chunk, "plies": plies, "played_share": table.occupancy() / 162,
            "min_value": int(values.min()), "max_value": int(values.max()),
            "heaviest": [{"colour": "bw"[e // 81], "move": go.unsquash(e % 81), "value": int(values[e]),
                          "played": int(counts[e, 0]), "won": int(counts[e, 1])}
                         for e in np.argsort(-values.astype(np.int64), kind="stable")[:10].tolist()],
            "black_win": black / n}


def move_contexts_report(recs, n, seed, chunk, rules="device", komi=L.KOMI, **kw):
    """move_values_report with a MoveContextTable of the default parameters -> a dict: the plies played, the
    share of plane 81's 162 entries with a play, the share of the 13,122 context entries with a play and with at least
    min_plays of them, the smallest and largest value of the whole table, its ten heaviest context entries and black's share
    of the wins."""
    table, plies, black = MoveContextTable.empty(), 0, 0
    ctr = default_counters(n, np.repeat(record_turns(recs), n))
    for s in range(0, n, chunk):
        c = min(chunk, n - s)
        fin = random_playouts(np.repeat(recs, c, 0), seed, counters=ctr[s:s + c], rules=rules, komi=komi, move_values=table, **kw)
        plies += int(fin.plies.sum())
        black += int((fin.score > 0).sum())
    values, counts = table.values, table.counts
    ctx = values[:, :81].astype(np.int64).reshape(-1)
    contexts = 2 * 81 * 81
    return {"playouts": n, "chunk": chunk, "plies": plies, "min_plays": table.min_plays,
            "played_share": int((counts[:, 81, :, 0] > 0).sum()) / 162,
            "context_played_share": int((counts[:, :81, :, 0] > 0).sum()) / contexts,
            "context_qualified_share": table.qualified() / contexts,
            "min_value": int(values.min()), "max_value": int(values.max()),
            "heaviest": [{"colour": "bw"[e // 6561], "after": go.unsquash(e // 81 % 81), "move": go.unsquash(e % 81),
                          "value": int(ctx[e]), "played": int(counts[e // 6561, e // 81 % 81, e % 81, 0]),
                          "won": int(counts[e // 6561, e // 81 % 81, e % 81, 1])}
                         for e in np.argsort(-ctx, kind="stable")[:10].tolist()],
            "black_win": black / n}


def main(argv=None):
    args = _parse(argv)
    game = sgf_position(args.sgf, args.move)
    torch.cuda.set_device(args.device)
    if args.amaf:
        recs = _as_records(game)
        a = playout_amaf(recs, args.n, args.seed, komi=args.komi, device=torch.device("cuda", args.device),
                         patterns=args.patterns, tactics=args.tactics, sides=args.sides)
        prior = amaf_prior(recs, a)[0]
        played, won = (a.played[0], a.won[0]) if args.sides == 1 else (a.played[0, 0], a.won[0, 0])
        out = {"value": float(a.value[0]), "wins": int(a.wins[0]), "playouts": args.n,
               "prior": [{"move": go.unsquash(s), "prior": float(prior[s]), "played": int(played[s]),
                          "won": int(won[s])} for s in np.argsort(-prior, kind="stable")[:10].tolist()]}
        if args.sides == 2:                                               # the opponent's points, by the playouts they were played in
            out["opponent"] = [{"move": go.unsquash(s), "played": int(a.played[0, 1, s]), "won": int(a.won[0, 1, s])}
                               for s in np.argsort(-a.played[0, 1], kind="stable")[:10].tolist()]
        print(json.dumps(out))
        return
    if args.weights:
        recs = _as_records(game)
        w = move_weights(recs, args.patterns, args.tactics, device=torch.device("cuda", args.device))[0]
        p = pattern_prior(recs, w[None])[0]
        print(json.dumps({"playable": int((w > 0).sum()),
                          "weights": [{"move": go.unsquash(s), "weight": int(w[s]), "share": float(p[s])}
                                      for s in np.argsort(-w, kind="stable")[:10].tolist() if w[s] > 0]}))
        return
    if args.replies:
        print(json.dumps(reply_report(_as_records(game), args.n, args.seed, args.chunk, komi=args.komi, patterns=args.patterns,
                                      tactics=args.tactics, device=torch.device("cuda", args.device))))
        return
    if args.reply_pairs:
        print(json.dumps(reply_pairs_report(_as_records(game), args.n, args.seed, args.chunk, komi=args.komi,
                                            patterns=args.patterns, tactics=args.tactics,
                                            device=torch.device("cuda", args.device))))
        return
    if args.move_values:
        print(json.dumps(move_values_report(_as_records(game), args.n, args.seed, args.chunk, komi=args.komi,
                                            patterns=args.patterns, tactics=args.tactics,
                                            device=torch.device("cuda", args.device))))
        return
    if args.move_contexts:
        print(json.dumps(move_contexts_report(_as_records(game), args.n, args.seed, args.chunk, komi=args.komi,
                                              patterns=args.patterns, tactics=args.tactics,
                                              device=torch.device("cuda", args.device))))
        return
    if args.ownership:
        o = playout_ownership(_as_records(game), args.n, args.seed, komi=args.komi, device=torch.device("cuda", args.device),
                              patterns=args.patterns, tactics=args.tactics)
        crit = o.criticality()[0]
        print(json.dumps({"value": float(o.value[0]), "black_wins": int(o.black_wins[0]), "playouts": args.n,
                          "mean_margin": float(o.mean_margin[0]),
                          "critical": [{"move": go.unsquash(s), "criticality": float(crit[s]),
                                        "owner": float(o.mean_owner[0, s])}
                                       for s in np.argsort(-crit, kind="stable")[:10].tolist()]}))
        print(owner_board(o.mean_owner[0]))
        return
    eng = None
    if args.p is not None:
        from .reinforce import policy_engine
        from .train import load_weights

        eng = policy_engine(load_weights(args.p), args.device, min(args.n, 4096))
    try:
        r = rollout_score([game], eng, n=args.n, seed=args.seed, komi=args.komi,
                          device=torch.device("cuda", args.device), one_launch=args.random, patterns=args.patterns,
                          tactics=args.tactics)[0]
    finally:
        if eng is not None:
            eng.close()
    print(json.dumps({"score": format_score(r.score), "black_win": r.black_win, "mean_score": r.mean_score,
                      "dead": [go.unsquash(s) for s in r.stones("dead")],
                      "seki": [go.unsquash(s) for s in r.stones("seki")], "playouts": args.n,
                      "unfinished": r.unfinished}))
    print(owner_board(r.mean_owner))


if __name__ == "__main__":
    main()

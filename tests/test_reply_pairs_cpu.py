"""Replies keyed by the last two moves (LGRF-2) without a GPU: the fold on hand-written histories, a numpy model
of the closed form the device update computes, the use rule in the host playouts, the Python surface, and what the header,
the bindings and the build say."""
import copy
import ctypes
import dataclasses
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, selfplay
from bokego_amd import lockstep as L
from bokego_amd import replies as RP
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS
from bokego_amd.playout_options import PlayoutOptions
from conftest import REPO
from test_amaf_cpu import seeded_tables, three_records
from test_pattern_prior_cpu import eyes_only_record, golden_records, ko_record
from test_replies_cpu import random_histories, start

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
PASS, NONE, NO = go.PASS, RO.MOVE_NONE, RP.NONE
SEED = 5
S = 81                                      # the plane of the single-move table


# records = 4, playouts = 3, max_plies = 8.  T[c][p2][p1] is a pair entry, T[c][S][p1] a single entry.  The mover of ply t has
# the colour (turn + t) & 1 and won the row when (won != 0) == (t even).
HAND2_RECS = np.stack([start(40, 0), start(12, 1), start(PASS, 2), start(go._NO_MOVE, 0)])
HAND2_MOVES = np.array([
    # record 0: black to move after 40
    [41, 42, 43, 44, 41, 42, 45, NONE],     # won.  t0 touches plane 81 only: [0][S][40] = 41; t1 white lost, p2 = 40 is the record's
                                            # last move: [1][40][41] holds 42, cleared, [1][S][41] holds 50, stays; t2 [0][S][42] =
                                            # [0][41][42] = 43; t3 nothing to clear; t4 [0][S][44] = [0][43][44] = 41; t5 nothing;
                                            # t6 the context (41, 42) again: [0][S][42] = [0][41][42] = 45, the later store
    [41, 42, 45, PASS, 46, 90, 47, 48],     # lost.  t0 [0][S][40] holds 41: cleared; t1 [1][S][41] = [1][40][41] = 42 (cleared
                                            # above, stored now); t2 [0][S][42] and [0][41][42] hold 45: both cleared; a pass; the
                                            # reply to a pass; 90; the reply to 90; t7 p2 = 90 is no point: [1][S][47] = 48 only
    [60, 61, PASS, 62, 63, NONE, 70, 71],   # won.  t0 [0][S][40] = 60 (a later store overrides the clearing); t1 [1][S][60] holds
                                            # 200, not 61: stays; a pass; the reply to a pass; t4 p2 is a pass: [0][S][62] = 63
                                            # only; the row ends at t5, and 70, 71 count for nothing
    # record 1: white to move after 12
    [13, 14, NONE, NONE, NONE, NONE, NONE, NONE],   # won (white).  t0 [1][S][12] = 13; t1 black lost: [0][S][13] and [0][12][13]
                                                    # hold 14, both cleared
    [NONE] * 8,                             # over on entry
    [13, 15, 16, NONE, NONE, NONE, NONE, NONE],     # lost.  t0 [1][S][12] holds 13: cleared; t1 [0][S][13] = [0][12][13] = 15;
                                                    # t2 [1][13][15] holds 16: cleared, [1][S][15] is empty
    # record 2: black to move after a pass
    [5, 6, 7, NONE, NONE, NONE, NONE, NONE],        # won.  t0 replies to a pass: nothing; t1 p2 is a pass, [1][S][5] is empty:
                                                    # nothing; t2 [0][S][6] = [0][5][6] = 7
    [NONE] * 8,
    [NONE] * 8,
    # record 3: black to move, no move before
    [7, 8, 9, NONE, NONE, NONE, NONE, NONE],        # lost.  t0 replies to no move; t1 p2 is no move: [1][S][7] = 8 only; t2
                                                    # [0][S][8] holds 9: cleared, [0][7][8] holds 10: stays
    [47, 49, NONE, NONE, NONE, NONE, NONE, NONE],   # lost.  t1 [1][S][47] = 49: the last record's store over record 0's 48
    [7, 30, NONE, NONE, NONE, NONE, NONE, NONE],    # lost.  t1 [1][S][7] = 30: the later row's store
], np.int16)
HAND2_WON = np.array([1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0], np.uint8)
HAND2_BEFORE = np.full((2, 82, 81), NO, np.uint8)
for (c, p2, p1), x in {(1, 40, 41): 42, (1, S, 41): 50, (1, S, 60): 200, (0, S, 13): 14, (0, 12, 13): 14, (1, 13, 15): 16,
                       (0, S, 8): 9, (0, 7, 8): 10, (0, 3, 3): 200, (1, S, 80): 81}.items():
    HAND2_BEFORE[c, p2, p1] = x
HAND2_AFTER = HAND2_BEFORE.copy()
for (c, p2, p1), x in {(0, S, 40): 60, (1, S, 41): 42, (0, S, 44): 41, (0, 43, 44): 41, (1, S, 47): 49, (0, S, 62): 63,
                       (0, S, 13): 15, (0, 12, 13): 15, (1, 13, 15): NO, (0, S, 6): 7, (0, 5, 6): 7, (1, S, 7): 30,
                       (0, S, 8): NO}.items():
    HAND2_AFTER[c, p2, p1] = x
HAND2_EVENTS = (20, 9, 10)                  # entries stored, cleared, left as they were


def random_table2(seed, points=12):
    rng = np.random.default_rng(seed)
    t = np.full((2, 82, 81), NO, np.uint8)
    t[:, :points, :points] = rng.integers(0, points, (2, points, points))
    t[:, S, :points] = rng.integers(0, points, (2, points))
    t[rng.random(t.shape) < 0.2] = NO
    t[0, 3, 3], t[1, S, 80], t[0, S, 2], t[1, 80, 80] = 200, 97, 81, 254   # invalid values: kept where nothing happens
    return t


def nine_records():
    """The nine records of test_gpu_replies.py: the board that needs no luck, the empty board, a record after a pass, two
    mid-game goldens (one per colour), the ko record, the eyes-only board, and two more goldens."""
    gold = golden_records()
    black = L.black_to_move(gold)
    mid = np.stack([gold[60], gold[61 + int(np.argmax(black[61:] != black[60]))]])
    recs = np.ascontiguousarray(np.concatenate([three_records(), mid, ko_record(), eyes_only_record(), gold[30:32]]))
    assert len(recs) == 9
    return recs


def learned2(recs, n, seed, **kw):
    """A pair table learned from n uniform playouts of each record, the counts of its update, and those playouts."""
    table = RO.ReplyTable2.empty()
    fin = RO.random_playouts(np.repeat(recs, n, 0), seed, counters=RO.value_counters(recs, n), rules="host", **kw)
    won = (fin.score > 0) == np.repeat(L.black_to_move(recs), n)
    events = RO.reply2_update_host(table, recs, fin.moves, won, len(recs), n)
    return table, events, fin


_LEARNED = {}


def learned_nine():
    """The table learned from four uniform playouts of each of the nine records, seed 5: computed once, never modified."""
    if not _LEARNED:
        _LEARNED["table"] = learned2(nine_records(), 4, SEED)[0]
    return _LEARNED["table"].copy()


# ---- 1. the fold -------------------------------------------------------------------------------------------------------------
def test_the_fold_on_hand_written_histories():
    t = HAND2_BEFORE.copy()
    assert RO.reply2_update_host(t, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3) == HAND2_EVENTS
    assert np.array_equal(t, HAND2_AFTER), np.argwhere(t != HAND2_AFTER)
    table = RO.ReplyTable2(HAND2_BEFORE)
    assert RO.reply2_update_host(table, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3) == HAND2_EVENTS
    assert np.array_equal(table.array, HAND2_AFTER) and HAND2_BEFORE[1, S, 60] == 200 == HAND2_AFTER[0, 3, 3]
    rows = np.repeat(HAND2_RECS, 3, 0)                                # as twelve records of one playout each: the same fold
    t = HAND2_BEFORE.copy()
    assert RO.reply2_update_host(t, rows, HAND2_MOVES, HAND2_WON, 12, 1) == HAND2_EVENTS and np.array_equal(t, HAND2_AFTER)
    # one event at a time, on the context (p2, p1) = (40, 41) of white at ply 1 of record 0
    for won, pair, single, pair_after, single_after in ((0, NO, NO, 42, 42), (1, 42, 42, NO, NO), (1, 42, 50, NO, 50),
                                                        (1, 43, 42, 43, NO), (0, 43, 50, 42, 42)):
        t = np.full((2, 82, 81), NO, np.uint8)
        t[1, 40, 41], t[1, S, 41] = pair, single
        RO.reply2_update_host(t, HAND2_RECS[:1], np.array([[90, NONE]], np.int16), [won], 1, 1)   # (a move above 80: nothing)
        assert t[1, 40, 41] == pair and t[1, S, 41] == single
        RO.reply2_update_host(t, HAND2_RECS[:1], np.array([[41, 42, NONE]], np.int16), [won], 1, 1)
        assert t[1, 40, 41] == pair_after and t[1, S, 41] == single_after
        t[1, 40, 41] = t[1, S, 41] = t[0, S, 40] = NO                 # (and ply 0 touched plane 81 only)
        assert (t == NO).all()
    with pytest.raises(ValueError):
        RO.reply2_update_host(t, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 2)
    with pytest.raises(ValueError):
        RO.reply2_update_host(np.full((2, 81), NO, np.uint8), HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3)


def closed_form(table, recs, moves, won, records, playouts):
    """The device update as a numpy model: per entry the key of its last store, max over (order + 1) << 8 | m; a flag where a
    loser's event would clear (with no store: its m equals the value on entry; else: it is later than the last store and
    its m equals the stored value); then one pass over the entries.  Nothing here depends on the order of the events."""
    lm0 = L.record_last_move(recs).astype(np.int64)
    c0 = (L.record_turns(recs) & 1).astype(np.int64)
    max_plies = moves.shape[1]
    events = []                                                       # (entry, order, m, mover_won)
    for row in range(len(moves)):
        r = row // playouts
        for k in range(max_plies):
            m = int(moves[row, k])
            if m <= NONE:
                break
            p1 = int(lm0[r]) if k == 0 else int(moves[row, k - 1])
            p2 = None if k == 0 else int(lm0[r]) if k == 1 else int(moves[row, k - 2])
            if not (0 <= m <= 80 and 0 <= p1 <= 80):
                continue
            c = int(c0[r]) ^ (k & 1)
            for plane in (S,) + ((p2,) if p2 is not None and 0 <= p2 <= 80 else ()):
                events.append(((c, plane, p1), row * max_plies + k, m, bool(won[row]) == (k % 2 == 0)))
    rng = np.random.default_rng(len(events))
    keys, flags = np.zeros((2, 82, 81), np.uint64), np.zeros((2, 82, 81), bool)
    for i in rng.permutation(len(events)):                            # any order
        e, order, m, wins = events[i]
        if wins:
            keys[e] = max(int(keys[e]), (order + 1) << 8 | m)
    for i in rng.permutation(len(events)):
        e, order, m, wins = events[i]
        if not wins:
            key = int(keys[e])
            if (key == 0 and int(table[e]) == m) or (key != 0 and order + 1 > key >> 8 and (key & 255) == m):
                flags[e] = True
    out = np.where(keys != 0, (keys & np.uint64(255)).astype(np.uint8), table)
    out[flags] = NO
    return out


def test_the_closed_form_equals_the_sequential_fold():
    assert np.array_equal(closed_form(HAND2_BEFORE, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3), HAND2_AFTER)
    rng = np.random.default_rng(26)
    for stream in range(40):
        records, playouts, max_plies = (int(rng.integers(1, hi + 1)) for hi in (4, 5, 39))
        recs, moves, won = random_histories(records, playouts, max_plies, 100 + stream, points=6)
        before = random_table2(stream, points=6)
        want = before.copy()
        RO.reply2_update_host(want, recs, moves, won, records, playouts)
        got = closed_form(before, recs, moves, won, records, playouts)
        assert np.array_equal(got, want), (stream, np.argwhere(got != want))


@pytest.mark.parametrize("records,playouts,max_plies", [(3, 5, 9), (1, 7, 30), (4, 1, 6)])
def test_plane_81_is_the_single_move_fold(records, playouts, max_plies):
    recs, moves, won = random_histories(records, playouts, max_plies, 11 + records)
    pairs, singles = random_table2(3), None
    singles = np.ascontiguousarray(pairs[:, S])
    before = pairs.copy()
    RO.reply2_update_host(pairs, recs, moves, won, records, playouts)
    RO.reply_update_host(singles, recs, moves, won, records, playouts)
    assert np.array_equal(pairs[:, S], singles) and not np.array_equal(pairs[:, :S], before[:, :S])
    assert pairs[0, 3, 3] == 200 and pairs[1, 80, 80] == 254
    t = RO.ReplyTable2(HAND2_BEFORE)
    single = t.singles()
    RO.reply2_update_host(t, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3)
    RO.reply_update_host(single, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3)
    assert np.array_equal(t.singles().array, single.array)


# ---- 2. the use rule -------------------------------------------------------------------------------------------------------------
def moves_of(recs, table, plies=1, seed=SEED, **kw):
    return RO.random_playouts(recs, seed, max_plies=plies, rules="host", replies=RO.ReplyTable2(table), **kw)


def test_a_pair_goes_before_a_single_and_both_only_where_playable():
    ko = ko_record()                                                  # white to move after black's 11; the ko point is 10
    plain = int(RO.random_playouts(ko, SEED, max_plies=1, rules="host").moves[0, 0])
    ok = RO.playable_host(ko)[0]
    good, other = (int(x) for x in np.nonzero(ok)[0][-2:])
    assert len({good, other, plain}) == 3 and not ok[10] and not ok[11]
    # reply2_moves itself, with a move two plies back of our choosing (white's 30)
    for pair, single, want, which in ((good, other, good, 2), (good, NO, good, 2), (10, other, other, 1), (11, other, other, 1),
                                      (81, other, other, 1), (200, other, other, 1), (NO, other, other, 1), (10, 11, -1, 0),
                                      (200, 81, -1, 0), (NO, NO, -1, 0)):
        t = np.full((2, 82, 81), NO, np.uint8)
        t[1, 30, 11], t[1, S, 11] = pair, single
        mv, by = RP.reply2_moves(t, ko, [30], ok[None])
        assert (int(mv[0]), int(by[0])) == (want, which), (pair, single)
        for p2 in (PASS, NONE, go._NO_MOVE, 81, 31):                  # no such pair: the single decides
            mv, by = RP.reply2_moves(t, ko, [p2], ok[None])
            assert (int(mv[0]), int(by[0])) == ((single, 1) if single == other else (-1, 0)), (pair, single, p2)
        t[0], t[1, 30, 11], t[1, S, 11] = t[1].copy(), NO, NO         # the other colour's entries are not asked
        assert RP.reply2_moves(t, ko, [30], ok[None])[0][0] == -1
    # in a playout, ply 0 has no move two plies back: every pair plane may say `good`, the single decides
    t = np.full((2, 82, 81), NO, np.uint8)
    t[:, :S] = good
    assert int(moves_of(ko, t).moves[0, 0]) == plain
    t[1, S, 11] = other
    fin = moves_of(ko, t)
    assert int(fin.moves[0, 0]) == other and fin.reply_plies == 1 and fin.reply_pair_plies == 0
    eyes = eyes_only_record()                                         # white to move after black's 38: eyes and suicides only
    lib = go.golib()
    own = [int(s) for s in np.nonzero(eyes[0, :81] == 0)[0] if lib.bk_pos_possible_eye(L.pos_ptr(eyes[0]), int(s)) == 2]
    t = np.full((2, 82, 81), own[0], np.uint8)                        # white's own one-point eye, everywhere
    assert int(moves_of(eyes, t).moves[0, 0]) == PASS
    mv, by = RP.reply2_moves(t, eyes, [30], RO.playable_host(eyes))
    assert int(mv[0]) == -1 and int(by[0]) == 0
    passed = three_records()[2:]                                      # the last move is a pass: nothing is asked
    plain = int(RO.random_playouts(passed, SEED, max_plies=1, rules="host").moves[0, 0])
    assert int(moves_of(passed, np.zeros((2, 82, 81), np.uint8)).moves[0, 0]) == plain and RO.playable_host(passed)[0, 0]


def test_ply_1_uses_the_records_last_move_as_p2():
    rec = golden_records()[60:61]
    lm0, c0 = int(L.record_last_move(rec)[0]), int(L.record_turns(rec)[0]) & 1
    plain = RO.random_playouts(rec, SEED, max_plies=2, rules="host")
    m0, m1 = (int(x) for x in plain.moves[0, :2])
    assert 0 <= lm0 <= 80 and 0 <= m0 <= 80
    ok = RO.playable_host(RO.random_playouts(rec, SEED, max_plies=1, rules="host").records)[0]   # after ply 0
    want = int([s for s in np.nonzero(ok)[0] if s != m1][0])
    t = np.full((2, 82, 81), NO, np.uint8)
    t[c0 ^ 1, lm0, m0] = want
    fin = moves_of(rec, t, plies=2)
    assert [int(x) for x in fin.moves[0, :2]] == [m0, want] and fin.reply_plies == 1 and fin.reply_pair_plies == 1
    t[c0 ^ 1, lm0, m0], t[c0, lm0, m0] = NO, want                     # the other colour's entry: not asked
    assert int(moves_of(rec, t, plies=2).moves[0, 1]) == m1


def test_all_255_pairs_play_the_single_tables_games():
    recs = np.concatenate([ko_record(), eyes_only_record(), three_records()[2:], golden_records()[60:61]])
    pat, tac = seeded_tables()
    single = learned_nine().singles()
    pairs = np.full((2, 82, 81), NO, np.uint8)
    pairs[:, S] = single.array
    for kw in (dict(), dict(patterns=pat), dict(tactics=tac), dict(patterns=pat, tactics=tac)):
        rows = np.repeat(recs, 2, 0)
        want = RO.random_playouts(rows, SEED, rules="host", replies=single.copy(), **kw)
        got = RO.random_playouts(rows, SEED, rules="host", replies=RO.ReplyTable2(pairs), **kw)
        assert got.reply_plies == want.reply_plies and got.reply_pair_plies == 0 and want.reply_plies > 0, sorted(kw)
        for f in ("records", "moves", "plies", "over", "score", "owner"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), (sorted(kw), f)
        a, b = single.copy(), RO.ReplyTable2(pairs)                   # and the run updates plane 81 as the single table
        RO.playout_value(recs, 2, SEED, rules="host", replies=a, **kw)
        RO.playout_value(recs, 2, SEED, rules="host", replies=b, **kw)
        assert np.array_equal(b.singles().array, a.array) and b.pairs_occupancy() > 0


def test_a_learned_table_decides_pair_plies():
    nine, table = nine_records(), learned_nine()
    assert table.pairs_occupancy() > 100 and table.singles().occupancy() > 20
    assert table.occupancy() == table.pairs_occupancy() + table.singles().occupancy()
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(9, RO.record_turns(nine)), 9)
    seen = {}
    for cap in (1, 2, 8, 400):
        fin = RO._random_host(nine, key, ctr, cap, L.KOMI, True, None, None, table.copy())
        pair, single = RP.reply2_plies_of(table, nine, fin.moves, 1)
        assert (pair, pair + single) == (fin.reply_pair_plies, fin.reply_plies), cap
        seen[cap] = (pair, single)
    print("pair and single plies by cap:", seen, "pair entries:", table.pairs_occupancy())
    assert seen[1][0] == 0                                            # ply 0 has no pair by definition
    assert seen[8][0] > 0 and seen[400][0] > 0 and seen[8][1] > 0 and seen[400][1] > 0
    with pytest.raises(TypeError, match="slots"):
        RO.random_playouts(nine, SEED, rules="host", replies=table.copy(), slots=np.zeros(9, np.int64))


# ---- 3. the table, the evaluator and the search -----------------------------------------------------------------------------------
def test_the_table_class():
    t = RO.ReplyTable2.empty()
    assert isinstance(t, RO.ReplyTable) and t.array.shape == (2, 82, 81) and t.array.dtype == np.uint8 and t.occupancy() == 0
    assert t.array.nbytes == 13284
    t.array[0, 5, 6], t.array[1, S, 7], t.array[1, S, 8] = 7, 8, 200
    assert t.occupancy() == 2 and t.pairs_occupancy() == 1
    s = t.singles()
    assert type(s) is RO.ReplyTable and s.array[1, 7] == 8 and s.occupancy() == 1 and not np.shares_memory(s.array, t.array)
    c = t.copy()
    c.array[0, 0, 0] = 3
    assert type(c) is RO.ReplyTable2 and t.array[0, 0, 0] == NO
    for again in (pickle.loads(pickle.dumps(t)), copy.deepcopy(t)):
        assert type(again) is RO.ReplyTable2 and np.array_equal(again.array, t.array)
    t.clear()
    assert t.occupancy() == 0
    for bad in (np.zeros((2, 81), np.uint8), np.zeros((2, 82, 81), np.int32), np.zeros((2, 81, 81), np.uint8)):
        with pytest.raises(ValueError):
            RO.ReplyTable2(bad)
    for name in ("ReplyTable2", "reply2_update_host", "reply_pairs_report"):
        assert name in RO.__all__
    rep = RO.reply_pairs_report(three_records()[1:2], 12, SEED, 4, rules="host")
    assert rep["playouts"] == 12 and rep["pair_plies"] + rep["single_plies"] < rep["plies"] and rep["single_plies"] > 0
    assert rep["pair_occupancy"] > 0 and rep["single_occupancy"] > 0
    assert RO.reply_pairs_report(three_records()[1:2], 12, SEED, 12, rules="host")["single_plies"] == 0


def _bits(out):
    return [np.asarray(x).tobytes() for x in out[:2]] + ([np.asarray(x).tobytes() for x in out[2][1:]] if len(out) > 2 else [])


def test_the_evaluator_with_a_pair_table():
    recs = np.concatenate([three_records()[1:], golden_records()[60:62]])
    same = lambda x: x                                                # noqa: E731
    base = dict(seed=4, rules="host", prior=1.0, rave=True)

    def three(ev):
        return [ev.finish(ev.submit(recs, 2), normalise=same) for _ in range(3)]

    ev = RO.PlayoutEvaluator(None, 6, replies=2, **base)
    assert type(ev.replies) is RO.ReplyTable2 and ev.replies.occupancy() == 0 and ev.wants_games is False
    runs = three(ev)
    plain = RO.PlayoutEvaluator(None, 6, **base)
    assert _bits(runs[0]) == _bits(plain.finish(plain.submit(recs, 2), normalise=same))   # the first request saw an empty table
    assert ev.replies.pairs_occupancy() > 0 and ev.replies.singles().occupancy() > 0
    table = ev.replies.copy()
    ev.reset_replies()
    assert ev.replies.occupancy() == 0
    assert [_bits(r) for r in three(ev)] == [_bits(r) for r in runs] and np.array_equal(ev.replies.array, table.array)
    assert [_bits(r) for r in three(RO.PlayoutEvaluator(None, 6, replies=2, **base))] == [_bits(r) for r in runs]
    old = RO.PlayoutEvaluator(None, 6, replies=True, **base)          # today's evaluator, as it is
    assert type(old.replies) is RO.ReplyTable
    single = three(old)
    want = RO.ReplyTable.empty()
    for k in range(3):
        run = RO._playouts(recs, 6, L.seed_u64(4), "host", counted=len(recs), sides=2, replies=want)
        assert np.array_equal(single[k][1], run.value) and run.reply_pair_plies is None
    assert np.array_equal(old.replies.array, want.array)
    with pytest.raises(TypeError, match="per game"):
        RO.PlayoutEvaluator(None, 6, replies=2, games=3, **base)
    with pytest.raises(TypeError):
        ev.submit(recs, 2, games=np.zeros(len(recs), np.int64))


def test_native_mcts_with_reply_pairs():
    def tree(seed=SEED, **kw):
        return NativeMCTS(None, None, None, playout_value=8, playout_prior=1, playout_reply_pairs=True, playout_rules="host",
                          playout_seed=seed, **kw)

    seen = []
    for seed in (SEED, SEED):
        t = tree(seed)
        assert t.playout_reply_pairs is True and t.playout_replies is False and type(t.evaluator.replies) is RO.ReplyTable2
        t.rollout(40)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move, t.evaluator.replies.array.copy()))
        if len(seen) == 2:
            c = copy.deepcopy(t)                                      # a table of its own, empty; the original's stays
            assert c.evaluator is not t.evaluator and c.evaluator.replies.occupancy() == 0 and c.playout_reply_pairs is True
            assert type(c.evaluator.replies) is RO.ReplyTable2 and c.evaluator.komi == t.evaluator.komi
            c.rollout(4)
            assert np.array_equal(t.evaluator.replies.array, seen[-1][2])
            c.close()
            p = pickle.loads(pickle.dumps(t))                         # rebuilds its evaluator, and an empty table, on first use
            assert p.evaluator is None and p.playout_reply_pairs is True
            p.rollout(1)
            assert type(p.evaluator.replies) is RO.ReplyTable2 and p.evaluator.replies is not t.evaluator.replies
            p.close()
        t.close()
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1] and np.array_equal(seen[0][2], seen[1][2])
    assert sum(seen[0][0].values()) == 40 and (seen[0][2][:, :S] != NO).any() and (seen[0][2][:, S] != NO).any()
    t = tree(playout_replies=True)                                    # pairs contain singles
    assert type(t.evaluator.replies) is RO.ReplyTable2
    t.close()
    t = NativeMCTS(None, None, None, playout_value=2, playout_prior=1, playout_rules="host")
    assert t.playout_reply_pairs is False and t.evaluator.replies is None
    t.close()
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(None, None, None, playout_reply_pairs=True, playout_prior=1)


def test_the_option_and_the_command_lines(capsys):
    assert PlayoutOptions(2, 3, "host").playout_reply_pairs is False
    assert "playout_reply_pairs" not in vars(PlayoutOptions()) and "playout_replies" not in vars(PlayoutOptions())
    with pytest.raises(TypeError):
        PlayoutOptions(playout_value=8, playout_reply_pairs=True)    # set by from_keywords, from_args or assignment
    names = [f.name for f in dataclasses.fields(PlayoutOptions)]
    assert names[-2:] == ["playout_reply_pairs", "playout_replies"]
    o = PlayoutOptions(playout_value=8)
    o.playout_reply_pairs = True
    assert o == PlayoutOptions.from_keywords(dict(playout_value=8, playout_reply_pairs=True)) and o != PlayoutOptions(playout_value=8)
    assert o.search_keywords() == dict(playout_value=8, playout_reply_pairs=True)
    assert o.evaluator_keywords() == dict(playouts=8, seed=0, rules="device", replies=2) and o.name_suffix() == "-mc8-lgr2"
    both = PlayoutOptions.from_keywords(dict(playout_value=8, playout_reply_pairs=True, playout_replies=True))
    assert both.evaluator_keywords()["replies"] == 2 and both.name_suffix() == "-mc8-lgr2"
    assert both.search_keywords() == dict(playout_value=8, playout_replies=True, playout_reply_pairs=True)
    only = PlayoutOptions.from_keywords(dict(playout_value=8, playout_replies=True))
    assert only.evaluator_keywords()["replies"] is True and only.name_suffix() == "-mc8-lgr"
    assert "replies" not in PlayoutOptions.from_keywords(dict(playout_value=8)).evaluator_keywords()
    with pytest.raises(TypeError, match="playout_value"):
        PlayoutOptions.from_keywords(dict(playout_reply_pairs=True))
    for mod in (gtp, match):
        a = mod.parse_args(["--playout-value", "8", "--playout-reply-pairs"])
        assert a.playout.playout_reply_pairs is True and a.playout.playout_replies is False
        assert a.playout.name_suffix().endswith("-lgr2")
        a = mod.parse_args(["--playout-value", "8", "--playout-reply-pairs", "--playout-replies"])
        assert a.playout.evaluator_keywords()["replies"] == 2
        assert mod.parse_args(["--playout-value", "8"]).playout.playout_reply_pairs is False
        with pytest.raises(SystemExit):
            mod.parse_args(["--playout-reply-pairs"])
        assert "--playout-value" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                   # one evaluator serves many games there
        selfplay.parse_args(["--playout-value", "8", "--playout-reply-pairs"])
    assert "--playout-reply-pairs" in capsys.readouterr().err and not hasattr(selfplay.parse_args([]), "playout_reply_pairs")
    with pytest.raises(SystemExit):
        selfplay.parse_args(["--playout-value", "8", "--playout-replies"])
    a = RO._parse(["--sgf", "g.sgf", "--random", "--reply-pairs", "-n", "64", "--chunk", "8"])
    assert a.reply_pairs is True and a.chunk == 8 and a.replies is False
    assert RO._parse(["--sgf", "g.sgf", "--random"]).reply_pairs is False
    for bad in (["--reply-pairs"], ["--random", "--reply-pairs", "--amaf"], ["--random", "--reply-pairs", "--replies"],
                ["--random", "--reply-pairs", "--chunk", "0"]):
        with pytest.raises(SystemExit):
            RO._parse(["--sgf", "g.sgf"] + bad)
    capsys.readouterr()


def test_gtp_clears_the_pair_table_with_the_board():
    from bokego_amd.mcts_native import Position
    g = gtp.NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=4, playout_value=2, playout_prior=1,
                      playout_reply_pairs=True, playout_rules="host")
    try:
        g.running = True
        assert g.send("genmove b").startswith("= ") and type(g.evaluator.replies) is RO.ReplyTable2
        assert g.evaluator.replies.occupancy() > 0
        assert g.send("clear_board") == "= \n\n" and g.evaluator.replies.occupancy() == 0
        assert g.send("genmove b").startswith("= ")
    finally:
        g.close()


# ---- 4. header, bindings, build -------------------------------------------------------------------------------------------------
def test_header_bindings_and_build_name_the_entry_points():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_reply2_playouts\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*const\s+uint8_t\s*\*\s*replies2\s*,\s*int\s+max_plies\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,"
                     r"\s*int32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+bkt_reply2_update\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*const\s+int16_t\s*\*\s*moves\s*,"
                     r"\s*int\s+max_plies\s*,\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*uint8_t\s*\*\s*replies2\s*,\s*void\s*\*\s*scratch\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bsize_t\s+bkt_reply2_scratch_bytes\s*\(\s*void\s*\)", code)
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("replies2 is uint8 [2][82][81], 13284 bytes, 4-byte aligned", "a misaligned pointer is BKT_ERR_ARG",
                   "replies2[c][p2][p1] with p2 < 81 is the reply of colour c to the opponent's move on p1 that followed c's own "
                   "move on p2", "Plane p2 == 81 is the LGRF-1 table: replies2[c][81][p1] is replies[c][p1]",
                   "compared before it indexes anything", "At ply 1, p2 is the record's last move",
                   "at ply 0 there is no p2, because a record holds one move",
                   "if p1 and p2 are board points and replies2[c][p2][p1] is a point of P, that is the move",
                   "else, if p1 is a board point and replies2[c][81][p1] is a point of P, that is the move",
                   "A pass or \"no move\" as p1 asks nothing; as p2 it skips the pair lookup only",
                   "The Philox word stays indexed by the ply", "a mover who won the row stores m",
                   "a mover who lost clears the entry if it holds m", "Entries without an event keep their value",
                   "bkt_reply2_scratch_bytes() = 119556 bytes", "replies2 == NULL or misaligned returns BKT_ERR_ARG"):
        assert " ".join(phrase.replace("*", " ").split()) in flat, phrase
    P, I, U64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t
    assert T.SYMBOLS["bkt_reply2_playouts"] == (I, [P, I, U64, P, P, P, P, I, P, P, P, P, P]) and callable(T.reply2_playouts)
    assert T.SYMBOLS["bkt_reply2_update"] == (I, [P, P, I, P, I, I, P, P, P]) and callable(T.reply2_update)
    assert T.SYMBOLS["bkt_reply2_scratch_bytes"] == (Z, [])
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        lib.bkt_reply2_scratch_bytes.restype = Z
        assert lib.bkt_abi_version() == 4 and lib.bkt_reply2_playouts and lib.bkt_reply2_update
        assert lib.bkt_reply2_scratch_bytes() == 13284 * 9 == 119556
    make = open(os.path.join(CSRC, "Makefile")).read()
    (rule,) = [l for l in make.splitlines() if l.startswith("$(TRAIN_OUT):")]
    assert "bk_playout_reply2.hip" in rule.split() and "bk_playout_reply.hip" in rule.split()
    (line,) = [l for l in make.splitlines() if l.startswith("\t") and "-o $@" in l and "bk_playout_pat.hip" in l]
    assert "bk_playout_reply2.hip" not in line and "-shared bk_train.hip bk_train_bf16.hip bk_playout_pat.hip -o" in line
    pat = open(os.path.join(CSRC, "bk_playout_pat.hip")).read()
    assert pat.index('#include "bk_playout_tac.hip"') < pat.index('#include "bk_playout_reply.hip"') \
        < pat.index('#include "bk_playout_reply2.hip"')
    own = open(os.path.join(CSRC, "bk_playout_reply2.hip")).read()
    assert not re.search(r"#include", own.split("namespace {")[0].replace("included as text", "")) and "float" not in own
    kernels = re.findall(r"__global__[^(]*?(\w+)\s*\(", own)
    assert len(kernels) == 6, kernels
    for name in kernels:                                              # existing tests pick kernels by these substrings
        for taken in ("reply_playouts_kernel", "reply_uniform_playouts_kernel", "reply_summaries_kernel", "reply_apply_kernel",
                      "random_playouts_kernel", "pattern_playouts_kernel", "tactical_playouts_kernel"):
            assert taken not in name, (name, taken)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernels_build_without_spills_or_scratch_at_the_tactical_kernels_occupancy(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]

    def fields(name):
        (block,) = [b for b in blocks if name in b.split()[0]]
        return {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in
                (("occupancy", r"Occupancy \[waves/SIMD\]"), ("vgprs", r" VGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                 ("sspill", r"SGPRs Spill"), ("vspill", r"VGPRs Spill"), ("lds", r"LDS Size \[bytes/block\]"))}

    tactical = fields("tactical_playouts_kernel")
    for name, wrapped in (("lgr2_playouts_kernel", "tactical_playouts_kernel"), ("lgr2_uniform_playouts_kernel", "random_playouts_kernel")):
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (name, f)
        assert f["occupancy"] >= tactical["occupancy"] >= 4, (name, f, tactical)
        assert f["vgprs"] <= 128 and f["lds"] <= fields(wrapped)["lds"] + 13312, (name, f)
    for name in ("lgr2_init_kernel", "lgr2_store_kernel", "lgr2_clear_kernel", "lgr2_finish_kernel"):
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (name, f)

"""MAST playouts (move values) without a GPU: the update mirror against the definition in Python integers and
fractions, the weight rule at its clamp and its floor, the host games, the table class, the Python surface, and what the
header, the bindings and the build say."""
import copy
import ctypes
import dataclasses
import itertools
import math
import os
import pickle
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, selfplay
from bokego_amd import lockstep as L
from bokego_amd import movevalues as MV
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from bokego_amd.mcts_native import NativeMCTS
from bokego_amd.playout_options import PlayoutOptions
from conftest import REPO
from test_amaf_cpu import seeded_tables
from test_game_pair_tables_cpu import OLD_KERNELS, kernels_of
from test_replies_cpu import random_histories, start
from test_reply_pairs_cpu import learned_nine, nine_records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
PASS, NONE = go.PASS, RO.MOVE_NONE
SEED = 5

# records = 2, playouts = 4, max_plies = 8: passes, MOVE_NONE tails, an entry above 80, a point played twice in one row (by
# one colour and by both), both turn parities.
HAND_RECS = np.stack([start(40, 0), start(12, 3)])
HAND_MOVES = np.array([
    [41, 42, 41, 42, 41, NONE, 70, 71],     # black retakes 41 twice, white 42 once; 70 and 71 lie behind the end
    [41, PASS, 90, 41, NONE, NONE, NONE, NONE],   # a pass, an entry above 80, and 41 by white this time
    [NONE] * 8,                             # over on entry
    [5, 6, 7, 8, 9, 10, 11, 12],            # the whole width
    [13, 14, 13, NONE, NONE, NONE, NONE, NONE],   # record 1: white moves first
    [PASS, PASS, NONE, NONE, NONE, NONE, NONE, NONE],
    [14, 13, 90, 200, 14, 13, 14, 13],
    [80, 0, NONE, NONE, NONE, NONE, NONE, NONE],
], np.int16)
HAND_WON = np.array([1, 0, 1, 0, 1, 0, 0, 1], np.uint8)


def definition(counts, recs, moves, won, records, playouts, lut, k, limit):
    """The header's update in Python integers -> (counts, values) as nested lists; counts is a nested list [2][81][2]."""
    counts = [[list(e) for e in side] for side in counts]
    for row in range(records * playouts):
        c0 = int(recs[row // playouts][L.OFF_TURN:L.OFF_TURN + 4].view(np.int32)[0]) & 1
        for t, m in enumerate(int(x) for x in moves[row]):
            if m <= NONE:
                break
            if 0 <= m <= 80:
                e = counts[c0 ^ (t & 1)][m]
                e[0] += 1
                e[1] += int((int(won[row]) != 0) == (t % 2 == 0))
    values = [[0] * 81 for _ in range(2)]
    for c, m in itertools.product(range(2), range(81)):
        e = counts[c][m]
        if limit > 0 and e[0] >= limit:
            s = next(s for s in range(64) if e[0] >> s < limit)
            e[0], e[1] = e[0] >> s, e[1] >> s
        i = math.floor(Fraction(64 * (2 * e[1] + k), 2 * (e[0] + k)))
        assert 0 <= i <= 64 and e[1] <= e[0]
        values[c][m] = int(lut[i])
    return counts, values


def table_of(counts=None, tau=0.25, k=16, limit=16384, lut=None):
    t = MV.MoveValueTable.empty(tau, k, limit)
    if lut is not None:
        t = MV.MoveValueTable(t.counts, np.full((2, 81), lut[32], np.uint16), lut, k, limit)
    if counts is not None:
        t.counts[...] = counts
    return t


def check(table, recs, moves, won, records, playouts):
    """One mirror update of `table` against the definition -> the number of plays."""
    want = definition(table.counts.tolist(), recs, moves, won, records, playouts, table.lut, table.k, table.limit)
    plays = MV.move_value_update_host(table, recs, moves, won, records, playouts)
    assert table.counts.tolist() == want[0] and table.values.tolist() == want[1]
    assert (table.counts[..., 1] <= table.counts[..., 0]).all() and (table.counts >= 0).all() and (table.values >= 1).all()
    return plays


def ramp_lut():
    return (np.arange(65) * 3 + 7).astype(np.uint16)                  # every i its own value: the index is visible


# ---- 1. the update ---------------------------------------------------------------------------------------------------------------
def test_the_update_on_hand_written_histories():
    t = table_of(lut=ramp_lut(), k=1, limit=0)
    assert check(t, HAND_RECS, HAND_MOVES, HAND_WON, 2, 4) == 5 + 2 + 0 + 8 + 3 + 0 + 6 + 2
    c = t.counts
    assert c[0, 41].tolist() == [4, 3] and c[1, 42].tolist() == [2, 0] and c[1, 41].tolist() == [1, 1]   # retaken points count again
    assert c[0, 70].tolist() == [0, 0] and c[1, 71].tolist() == [0, 0]                                   # behind the end
    assert c[1, 13].tolist() == [2, 2] and c[0, 14].tolist() == [1, 0]                                   # record 1: white first
    assert c[1, 14].tolist() == [3, 0] and c[0, 13].tolist() == [3, 3] and c[1, 80].tolist() == [1, 1] and c[0, 0].tolist() == [1, 0]
    assert int(c[..., 0].sum()) == 26
    assert t.values[0, 41] == ramp_lut()[64 * 7 // 10] and t.values[1, 42] == ramp_lut()[64 * 1 // 6] and t.values[0, 70] == ramp_lut()[32]


@pytest.mark.parametrize("max_plies", [1, 8])
@pytest.mark.parametrize("records,playouts", [(1, 1), (1, 3), (2, 4)])
def test_the_mirror_equals_the_definition(records, playouts, max_plies):
    rows = records * playouts
    recs, moves, won = HAND_RECS[2 - records:], HAND_MOVES[8 - rows:, :max_plies], HAND_WON[8 - rows:]
    for k, limit in ((1, 0), (16, 16384), (65536, 0), (3, 4), (1, 2)):
        rng = np.random.default_rng(k + limit)
        before = np.zeros((2, 81, 2), np.int64)
        before[..., 0] = rng.integers(0, max(limit, 50), (2, 81))
        before[..., 1] = rng.integers(0, 1 << 30, (2, 81)) % (before[..., 0] + 1)
        for counts in (None, before):
            check(table_of(counts, k=k, limit=limit, lut=ramp_lut()), recs, moves, won, records, playouts)
    recs, moves, won = random_histories(records, playouts, max_plies, 11 * rows + max_plies)
    assert check(table_of(lut=ramp_lut(), k=2, limit=0), recs, moves, won, records, playouts) >= 0


def test_the_order_of_rows_and_records_does_not_matter_and_two_calls_equal_one():
    recs, moves, won = random_histories(3, 5, 20, 7)
    one = table_of(k=4, limit=0)
    check(one, recs, moves, won, 3, 5)
    rng = np.random.default_rng(1)
    within = np.concatenate([r * 5 + rng.permutation(5) for r in range(3)])      # the rows of a record among themselves
    a = table_of(k=4, limit=0)
    MV.move_value_update_host(a, recs, moves[within], won[within], 3, 5)
    order = np.array([2, 0, 1])                                                   # the records
    rows = (order[:, None] * 5 + np.arange(5)[None, :]).reshape(-1)
    b = table_of(k=4, limit=0)
    MV.move_value_update_host(b, recs[order], moves[rows], won[rows], 3, 5)
    two = table_of(k=4, limit=0)                                                  # no shift: two calls add up
    MV.move_value_update_host(two, recs[:1], moves[:5], won[:5], 1, 5)
    MV.move_value_update_host(two, recs[1:], moves[5:], won[5:], 2, 5)
    for t in (a, b, two):
        assert np.array_equal(t.counts, one.counts) and np.array_equal(t.values, one.values)
    assert one.occupancy() > 10 and len(set(one.values.reshape(-1).tolist())) > 3


@pytest.mark.parametrize("limit", [2, 4])
def test_a_small_limit_forgets_and_the_sequence_of_calls_matters(limit):
    recs, moves, won = random_histories(2, 6, 12, 3)
    one = table_of(k=1, limit=limit, lut=ramp_lut())
    check(one, recs, moves, won, 2, 6)
    two = table_of(k=1, limit=limit, lut=ramp_lut())
    check(two, recs[:1], moves[:6], won[:6], 1, 6)
    check(two, recs[1:], moves[6:], won[6:], 1, 6)
    assert (one.counts[..., 0] < limit).all() and (two.counts[..., 0] < limit).all()
    assert not np.array_equal(one.counts, two.counts)                 # halved in between: as defined, and checked against it
    free = table_of(k=1, limit=0, lut=ramp_lut())
    check(free, recs, moves, won, 2, 6)
    assert free.counts[..., 0].max() >= 4 and not np.array_equal(free.counts, one.counts)


def test_the_rate_index_on_a_grid_with_its_ends():
    for k in (1, 2, 16, 1000, 65536):
        for played in (0, 1, 2, 3, 7, 64, 1000, 16383, (1 << 30) - 1, 1 << 40):
            for won in sorted(w for w in {0, 1, played // 3, played // 2, played - 1, played} if 0 <= w <= played):
                want = math.floor(Fraction(64 * (2 * won + k), 2 * (played + k)))
                assert int(MV.rate_index(played, won, k)) == want and 0 <= want <= 64, (k, played, won)
        assert int(MV.rate_index(0, 0, k)) == 32
    assert int(MV.rate_index(5, 5, 1)) == 58 and int(MV.rate_index(1 << 40, 1 << 40, 1)) == 63
    assert int(MV.rate_index(1 << 30, 0, 1)) == 0 and int(MV.rate_index(1 << 30, 1 << 30, 65536)) == 63
    assert int(MV.rate_index(64, 64, 1)) == 63 and int(MV.rate_index(0, 0, 7)) == 32
    # 64 itself needs won > played, which no table holds: the kernel compares before it indexes all the same
    assert int(MV.rate_index(1, 2, 1)) == 80 and np.minimum(MV.rate_index(1, 2, 1), 64) == 64


# ---- 2. the weight rule ----------------------------------------------------------------------------------------------------------
def test_the_weight_rule_neutral_at_the_clamp_and_at_the_floor():
    recs = nine_records()
    pat, tac = seeded_tables()
    c = RO.record_turns(recs) & 1
    for p, t in ((None, None), (pat, None), (None, tac), (pat, tac)):
        w = RO.move_weights_host(recs, p, t)
        neutral = MV.move_value_weights(w, np.full((2, 81), 256, np.uint16), c)
        assert np.array_equal(np.where(w > 0, neutral, 0), w)         # values all 256: move_weights_host's weights
    top_p, top_t = PT.PatternTable(np.full(PT.ENTRIES, 65535, np.uint16)), TC.TacticTable(np.full(TC.ENTRIES, 65535, np.uint16))
    w = RO.move_weights_host(recs, top_p, top_t)
    assert w.max() == (65535 * 65535) >> 8 == 16776704
    values = np.full((2, 81), 256, np.uint16)
    values[0], values[1, ::2] = 65535, 257
    got = MV.move_value_weights(w, values, c)
    black, white = np.nonzero(c == 0)[0], np.nonzero(c == 1)[0]
    assert (16776704 * 65535) >> 8 > (1 << 24) - 1 and (16776704 * 257) >> 8 > (1 << 24) - 1
    assert (got[black][w[black] > 0] == (1 << 24) - 1).all() and len(black) and len(white)
    assert (got[white][:, ::2][w[white][:, ::2] > 0] == (1 << 24) - 1).all() and (got[white][:, 1::2][w[white][:, 1::2] > 0] == 16776704).all()
    assert got.dtype == np.uint64 and int(got.max()) * 81 < 1 << 31
    low_p, low_t = PT.PatternTable(np.full(PT.ENTRIES, 1, np.uint16)), TC.TacticTable(np.full(TC.ENTRIES, 300, np.uint16))
    w = RO.move_weights_host(recs, low_p, low_t)
    assert set(np.unique(w).tolist()) == {0, 1}                       # (1 * 300) >> 8
    assert (MV.move_value_weights(w, np.full((2, 81), 1, np.uint16), c) == 1).all()      # (1 * 1) >> 8 = 0: the floor
    assert (MV.move_value_weights(np.full((9, 81), 255), np.full((2, 81), 1, np.uint16), c) == 1).all()
    assert (MV.move_value_weights(np.full((9, 81), 256), np.full((2, 81), 1, np.uint16), c) == 1).all()
    assert (MV.move_value_weights(np.full((9, 81), 1000), np.full((2, 81), 300, np.uint16), c) == 1171).all()
    with pytest.raises(ValueError):
        MV.move_value_weights(w, np.full((2, 81), 256, np.int16), c)


# ---- 3. the games ----------------------------------------------------------------------------------------------------------------
def same_games(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("records", "moves", "plies", "over", "score"))


def learned_values(seed=3):
    """A table with learned counts and a sharp lut, so that the games differ: 8 uniform playouts of the nine records."""
    t = MV.MoveValueTable.empty(tau=0.05, k=1, limit=0)
    RO.playout_value(nine_records(), 8, seed, rules="host", move_values=t)
    return t


def test_neutral_values_play_the_games_of_every_draw_and_learned_ones_do_not():
    recs = nine_records()
    pat, tac = seeded_tables()
    for kw in (dict(), dict(patterns=pat, tactics=tac), dict(replies=lambda: RO.ReplyTable(np.ascontiguousarray(learned_nine().array[:, 81]))),
               dict(patterns=pat, replies=learned_nine)):
        make = kw.pop("replies", None)
        r1, r2 = (None, None) if make is None else (make(), make())
        plain = RO.random_playouts(recs, SEED, rules="host", replies=r1, **kw)
        t = MV.MoveValueTable.empty()
        valued = RO.random_playouts(recs, SEED, rules="host", replies=r2, move_values=t, **kw)
        assert same_games(plain, valued) and t.occupancy() > 100, list(kw)
        assert r1 is None or np.array_equal(r1.array, r2.array)       # the reply table learned the same
        want = MV.MoveValueTable.empty()
        won = (plain.score > 0) == L.black_to_move(recs)
        MV.move_value_update_host(want, recs, plain.moves, won, 9, 1)
        assert np.array_equal(t.counts, want.counts) and np.array_equal(t.values, want.values)
    learned = learned_values()
    assert learned.values.min() < 100 and learned.values.max() > 600
    a, b = (RO.random_playouts(recs, SEED, rules="host", patterns=pat, tactics=tac, move_values=learned.copy()) for _ in range(2))
    assert same_games(a, b) and not same_games(a, RO.random_playouts(recs, SEED, rules="host", patterns=pat, tactics=tac))
    v = [RO.playout_value(recs, 4, SEED, rules="host", move_values=t) for t in (learned.copy(), learned.copy(), None)]
    assert np.array_equal(v[0], v[1]) and not np.array_equal(v[0], v[2])
    am = RO.playout_amaf(recs, 4, SEED, rules="host", move_values=learned.copy(), sides=2)
    assert np.array_equal(am.value, v[0]) and am.played.shape == (9, 2, 81)
    history = RO.random_playouts(recs, SEED, rules="host", move_values=MV.MoveValueTable.empty(), history=False)
    assert history.moves is None


def test_the_refusals_of_the_playout_functions():
    recs = nine_records()[:3]
    t = MV.MoveValueTable.empty()
    with pytest.raises(ValueError, match="move-value"):
        RO.playout_ownership(recs, 2, SEED, rules="host", move_values=t)
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", replies=RO.ReplyTables(2), slots=np.array([0, 1, 0]), move_values=t)
    with pytest.raises(TypeError, match="slots"):
        RO.random_playouts(recs, SEED, rules="host", replies=RO.ReplyTables2(2), slots=np.array([0, 1, 0]), move_values=t)
    with pytest.raises(TypeError, match="MoveValueTable"):
        RO.playout_value(recs, 2, SEED, rules="host", move_values=np.full((2, 81), 256, np.uint16))
    assert t.occupancy() == 0


# ---- 4. lut_of and the table class -----------------------------------------------------------------------------------------------
def test_lut_of_by_hand_at_three_tau():
    for tau in (0.25, 0.1, 1.0, 0.01, 1e6):
        lut = MV.lut_of(tau)
        assert lut.dtype == np.uint16 and lut.shape == (65,) and lut[32] == 256 and lut.min() >= 1
        assert (np.diff(lut.astype(np.int64)) >= 0).all()
    a = MV.lut_of(0.25)
    assert [int(a[i]) for i in (0, 16, 32, 48, 64)] == [35, 94, 256, 696, 1892]          # 256 e^-2, e^-1, 1, e, e^2
    b = MV.lut_of(0.1)
    assert [int(b[i]) for i in (0, 31, 33, 64)] == [2, 219, 299, 37994]                  # 256 e^-5, e^(-1/6.4), e^(1/6.4), e^5
    c = MV.lut_of(0.01)
    assert c[0] == 1 and c[64] == 65535 and c[33] == 1221                                 # clipped at both ends; 256 e^(100/64)
    assert (MV.lut_of(1e6) == 256).all()
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            MV.lut_of(bad)


def test_the_table_class_copies_clears_and_pickles():
    t = learned_values()
    assert t.k == 1 and t.limit == 0 and t.occupancy() > 100 and np.array_equal(t.lut, MV.lut_of(0.05))
    for other in (t.copy(), copy.deepcopy(t), pickle.loads(pickle.dumps(t)), copy.deepcopy({"x": t})["x"]):
        assert other is not t and type(other) is MV.MoveValueTable and (other.k, other.limit) == (1, 0)
        assert all(np.array_equal(getattr(other, f), getattr(t, f)) for f in ("counts", "values", "lut"))
        other.counts[0, 0, 0] += 1
        assert other.counts[0, 0, 0] == t.counts[0, 0, 0] + 1
    before = t.counts.copy()
    u = t.copy()
    u.clear()
    assert not u.counts.any() and (u.values == 256).all() and u.occupancy() == 0 and np.array_equal(t.counts, before)
    e = MV.MoveValueTable.empty()
    assert (e.k, e.limit) == (16, 16384) == (MV.DEFAULT_K, MV.DEFAULT_LIMIT) and MV.DEFAULT_TAU == 0.25
    assert np.array_equal(e.lut, MV.lut_of(0.25)) and not e.counts.any() and (e.values == 256).all()
    with pytest.raises(ValueError):
        e.lut[0] = 3                                                  # the lut is the table's for good
    zeros, neutral, lut = np.zeros((2, 81, 2), np.int64), np.full((2, 81), 256, np.uint16), MV.lut_of(1.0)
    for bad in (dict(counts=zeros.astype(np.int32)), dict(counts=zeros[:, :80]), dict(values=neutral.astype(np.int16)),
                dict(values=np.zeros((2, 81), np.uint16)), dict(lut=lut[:64]), dict(lut=np.zeros(65, np.uint16)), dict(k=0),
                dict(k=65537), dict(limit=1), dict(limit=-4), dict(limit=(1 << 30) + 1), dict(counts=zeros - 1),
                dict(counts=zeros + np.array([1, 2]))):
        with pytest.raises(ValueError):
            MV.MoveValueTable(**{**dict(counts=zeros, values=neutral, lut=lut, k=1, limit=0), **bad})
    assert MV.MoveValueTable(zeros, neutral, lut, 65536, 1 << 30).limit == 1 << 30 and MV.MoveValueTable(zeros, neutral, lut, 1, 2).limit == 2


def test_the_domain_of_the_host_update():
    recs, moves, won = random_histories(2, 3, 8, 1)
    t = MV.MoveValueTable.empty()
    for args in ((recs, moves, won, 3, 2), (recs, moves, won, 0, 6), (recs, moves, won, 2, 0), (recs, moves[:5], won[:5], 2, 3),
                 (recs, moves, won[:5], 2, 3), (recs[:1], moves, won, 2, 3), (recs, moves.reshape(-1), won, 2, 3),
                 (recs, np.zeros((6, 1025), np.int16), won, 2, 3), (recs, np.zeros((6, 0), np.int16), won, 2, 3)):
        with pytest.raises(ValueError):
            MV.move_value_update_host(t, *args)
    with pytest.raises(TypeError):
        MV.move_value_update_host(t.values, recs, moves, won, 2, 3)
    assert t.occupancy() == 0


# ---- 5. the evaluator, the options, the front ends --------------------------------------------------------------------------------
def test_the_evaluator_keeps_a_table_and_its_first_request_is_the_plain_one():
    recs = nine_records()[[1, 3, 4]]
    same = lambda x: x                                                # noqa: E731
    for more in (dict(), dict(replies=True), dict(replies=2, rave=True)):
        plain = RO.PlayoutEvaluator(None, 4, seed=SEED, rules="host", prior=1.0, **more)
        ev = RO.PlayoutEvaluator(None, 4, seed=SEED, rules="host", prior=1.0, move_values=True, **more)
        assert type(ev.move_values) is MV.MoveValueTable and plain.move_values is None and ev.move_values.occupancy() == 0
        a, b = plain.finish(plain.submit(recs, 1), normalise=same), ev.finish(ev.submit(recs, 1), normalise=same)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[:2], b[:2])) and ev.move_values.occupancy() > 50
        plays = int(ev.move_values.counts[..., 0].sum())
        ev.finish(ev.submit(recs, 1), normalise=same)                 # the table carries on from request to request
        assert int(ev.move_values.counts[..., 0].sum()) > plays and not (ev.move_values.values == 256).all()
        ev.reset_move_values()
        assert ev.move_values.occupancy() == 0 and (ev.move_values.values == 256).all()
    ev = RO.PlayoutEvaluator(None, 4, seed=SEED, rules="host", prior=1.0, move_values=0.1)
    assert np.array_equal(ev.move_values.lut, MV.lut_of(0.1)) and (ev.move_values.k, ev.move_values.limit) == (16, 16384)
    for bad in (dict(replies=True, games=2), dict(pair_games=2)):
        with pytest.raises(TypeError, match="move_values"):
            RO.PlayoutEvaluator(None, 4, rules="host", prior=1.0, move_values=True, **bad)
    with pytest.raises(ValueError, match="tau"):
        RO.PlayoutEvaluator(None, 4, rules="host", prior=1.0, move_values=-0.5)
    with pytest.raises(TypeError, match="move_values"):
        RO.PlayoutEvaluator(None, 4, rules="host", prior=1.0).reset_move_values()


def test_the_option_and_the_command_lines(capsys):
    assert PlayoutOptions(2, 3, "host").playout_move_values == 0.0 and "playout_move_values" not in vars(PlayoutOptions())
    with pytest.raises(TypeError):
        PlayoutOptions(playout_value=8, playout_move_values=0.25)    # set by from_keywords, from_args or assignment
    names = [f.name for f in dataclasses.fields(PlayoutOptions)]
    assert names[-3:] == ["playout_move_values", "playout_reply_pairs", "playout_replies"]
    o = PlayoutOptions(playout_value=8)
    o.playout_move_values = 0.5
    assert o == PlayoutOptions.from_keywords(dict(playout_value=8, playout_move_values=0.5)) and o != PlayoutOptions(playout_value=8)
    assert o.search_keywords() == dict(playout_value=8, playout_move_values=0.5)
    assert o.evaluator_keywords() == dict(playouts=8, seed=0, rules="device", move_values=0.5) and o.name_suffix() == "-mc8-mast"
    both = PlayoutOptions.from_keywords(dict(playout_value=8, playout_reply_pairs=True, playout_move_values=0.25, playout_rave=4))
    assert both.evaluator_keywords() == dict(playouts=8, seed=0, rules="device", rave=True, replies=2, move_values=0.25)
    assert both.name_suffix() == "-mc8-rave4-lgr2-mast"
    plain = PlayoutOptions.from_keywords(dict(playout_value=8))
    assert "move_values" not in plain.evaluator_keywords() and "playout_move_values" not in plain.search_keywords()
    assert plain.name_suffix() == "-mc8"
    with pytest.raises(TypeError, match="playout_move_values.*playout_value"):
        PlayoutOptions.from_keywords(dict(playout_move_values=0.25))
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="playout_move_values"):
            PlayoutOptions.from_keywords(dict(playout_value=8, playout_move_values=bad))
    for mod in (gtp, match):
        a = mod.parse_args(["--playout-value", "8", "--playout-prior", "1", "--playout-move-values"])
        assert a.playout.playout_move_values == 0.25 and a.playout.name_suffix().endswith("-mast")
        a = mod.parse_args(["--playout-value", "8", "--playout-prior", "1", "--playout-move-values", "0.1", "--playout-reply-pairs"])
        assert a.playout.evaluator_keywords()["move_values"] == 0.1 and a.playout.evaluator_keywords()["replies"] == 2
        assert mod.parse_args(["--playout-value", "8", "--playout-prior", "1"]).playout.playout_move_values == 0.0
        for argv, named in ((["--playout-move-values"], "--playout-value"), (["--playout-value", "8", "--playout-move-values", "-1"], "--playout-move-values"),
                            (["--playout-value", "8", "--playout-move-values", "nan"], "--playout-move-values")):
            with pytest.raises(SystemExit):
                mod.parse_args(argv)
            err = capsys.readouterr().err
            assert named in err and "--playout-move-values" in err
    with pytest.raises(SystemExit):                                   # one evaluator serves many games there
        selfplay.parse_args(["--playout-value", "8", "--playout-move-values"])
    assert "--playout-move-values" in capsys.readouterr().err and not hasattr(selfplay.parse_args([]), "playout_move_values")
    import argparse
    ap = argparse.ArgumentParser()
    PlayoutOptions.add_arguments(ap)
    text = " ".join(ap.format_help().split())
    assert "--playout-move-values [TAU]" in text and "untuned" in text.split("--playout-move-values [TAU]")[1]
    a = RO._parse(["--sgf", "g.sgf", "--random", "--move-values", "-n", "64", "--chunk", "8"])
    assert a.move_values is True and a.chunk == 8 and RO._parse(["--sgf", "g.sgf", "--random"]).move_values is False
    for bad in (["--move-values"], ["--random", "--move-values", "--amaf"], ["--random", "--move-values", "--replies"],
                ["--random", "--move-values", "--reply-pairs"], ["--random", "--move-values", "--chunk", "0"]):
        with pytest.raises(SystemExit):
            RO._parse(["--sgf", "g.sgf"] + bad)
    capsys.readouterr()
    rep = RO.move_values_report(nine_records()[1:2], 8, SEED, 4, rules="host")
    assert rep["playouts"] == 8 and 0 < rep["played_share"] <= 1 and rep["min_value"] < 256 < rep["max_value"] and len(rep["heaviest"]) == 10
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "--playout-move-values" in readme and "## 30." in open(os.path.join(REPO, "DESIGN.md")).read()


def test_native_mcts_and_gtp_keep_the_table_with_the_search():
    from bokego_amd.mcts_native import Position
    seen = []
    for _ in range(2):
        t = NativeMCTS(None, None, None, playout_value=2, playout_prior=1, playout_rules="host", playout_move_values=0.25,
                       playout_replies=True, playout_seed=SEED)
        assert t.playout_move_values == 0.25 and type(t.evaluator.move_values) is MV.MoveValueTable
        t.rollout(12)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.evaluator.move_values.counts.copy()))
        twin = copy.deepcopy(t)
        assert twin.evaluator is not t.evaluator and twin.evaluator.move_values.occupancy() == 0
        twin.close()
        t.close()
    assert seen[0][0] == seen[1][0] and np.array_equal(seen[0][1], seen[1][1]) and seen[0][1].any()
    t = NativeMCTS(None, None, None, playout_value=2, playout_prior=1, playout_rules="host")
    assert t.playout_move_values == 0.0 and t.evaluator.move_values is None
    t.close()
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(None, None, None, playout_move_values=0.25, playout_prior=1)
    g = gtp.NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=4, playout_value=2, playout_prior=1,
                      playout_move_values=0.25, playout_rules="host")
    try:
        g.running = True
        assert g.send("genmove b").startswith("= ") and g.evaluator.move_values.occupancy() > 0
        assert g.send("clear_board") == "= \n\n" and g.evaluator.move_values.occupancy() == 0
        assert g.send("genmove b").startswith("= ")
    finally:
        g.close()


# ---- 6. header, bindings, build ---------------------------------------------------------------------------------------------------
def test_header_bindings_makefile_and_the_kernels_names():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    for name, value in (("BKT_MOVE_VALUE_NEUTRAL", "256"), ("BKT_MOVE_VALUE_MAX_K", "65536"), ("BKT_MOVE_VALUE_MAX_LIMIT", r"\(1 << 30\)")):
        assert re.search(rf"#define\s+{name}\s+{value}", src), name
    assert (T.MOVE_VALUE_MAX_K, T.MOVE_VALUE_MAX_LIMIT) == (65536, 1 << 30) == (MV.MAX_K, MV.MAX_LIMIT)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_move_value_playouts\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*const\s+uint16_t\s*\*\s*values\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*replies\s*,\s*const\s+uint8_t\s*\*\s*replies2\s*,\s*int\s+max_plies\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,"
                     r"\s*int32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bsize_t\s+bkt_move_value_scratch_bytes\s*\(\s*int\s+records\s*\)", code)
    assert re.search(r"\bint\s+bkt_move_value_update\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*const\s+int16_t\s*\*\s*moves\s*,"
                     r"\s*int\s+max_plies\s*,\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*int64_t\s*\*\s*counts\s*,\s*uint16_t\s*\*\s*values\s*,\s*const\s+uint16_t\s*\*\s*lut\s*,\s*int\s+k\s*,"
                     r"\s*int\s+limit\s*,\s*void\s*\*\s*scratch\s*,\s*void\s*\*\s*stream\s*\)", code)
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("counts int64 [2][81][2]", "values uint16 [2][81]", "lut uint16 [65]",
                   "w = min(2^24 - 1, max(1, ((uint64_t)w_in * values[c][q]) >> 8))", "at most one of the two may be given",
                   "c = (colour to move at record r) xor (t & 1)", "there is no first-play rule",
                   "shifted right by the smallest s with played >> s < limit",
                   "i = floor(64 * (2 * won + k) / (2 * (played + k)))", "Every entry of values is written", "No wrap.",
                   "records * 1296 bytes", "a refused call launches nothing and writes nothing"):
        assert " ".join(phrase.replace("*", " ").split()) in flat, phrase
    P, I, U64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t
    assert T.SYMBOLS["bkt_move_value_playouts"] == (I, [P, I, U64, P, P, P, P, P, P, I, P, P, P, P, P]) and callable(T.move_value_playouts)
    assert T.SYMBOLS["bkt_move_value_update"] == (I, [P, P, I, P, I, I, P, P, P, I, I, P, P]) and callable(T.move_value_update)
    assert T.SYMBOLS["bkt_move_value_scratch_bytes"] == (Z, [I])
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        lib.bkt_move_value_scratch_bytes.restype, lib.bkt_move_value_scratch_bytes.argtypes = Z, [I]
        assert lib.bkt_abi_version() == 4 and lib.bkt_move_value_playouts and lib.bkt_move_value_update
        assert [lib.bkt_move_value_scratch_bytes(n) for n in (-1, 0, 1, 3, 1024)] == [0, 0, 1296, 3888, 1024 * 1296]
    # the Makefile: the draw's file a dependency only, the update's a source in front of -shared
    make = open(os.path.join(CSRC, "Makefile")).read()
    rule, line = re.search(r"^\$\(TRAIN_OUT\):(.*)\n\t(.*)$", make, flags=re.M).groups()
    assert "bk_playout_mast.hip" in rule.split() and "bk_playout_mast.hip" not in line.split()
    assert "bk_playout_mast_update.hip" in rule.split() and "bk_playout_mast_update.hip" in line.split("-shared")[0].split()
    assert "-shared bk_train.hip bk_train_bf16.hip bk_playout_pat.hip -o" in line
    # included as text at the very end of bk_playout_reply2_tables.hip: the chain's last two includes stay where they are
    host = open(os.path.join(CSRC, "bk_playout_reply2_tables.hip")).read()
    assert re.findall(r'^#include "([^"]+)"', host, flags=re.M) == ["bk_playout_mast.hip"]
    assert host.rstrip().splitlines()[-1].startswith('#include "bk_playout_mast.hip"')
    includes = re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, "bk_playout_pat.hip")).read(), flags=re.M)
    assert includes[-2:] == ["bk_playout_reply2.hip", "bk_playout_reply2_tables.hip"]
    draw, update = (open(os.path.join(CSRC, name)).read() for name in ("bk_playout_mast.hip", "bk_playout_mast_update.hip"))
    for own in (draw, update):
        assert "float" not in own and "double" not in own and not re.search(r"\batomic\w*\s*\(", own)
    assert "__syncthreads" not in draw and "#include" not in draw.split("namespace {")[0].replace("included as text", "")
    for inst in ("WeightedDraw<MoveValueWeight>", "ReplyDraw<WeightedDraw<MoveValueWeight>, 1>", "Reply2Draw<WeightedDraw<MoveValueWeight>>"):
        assert inst in draw, inst
    new = kernels_of("bk_playout_mast.hip") + kernels_of("bk_playout_mast_update.hip")
    assert len(new) == 5 and len(set(new)) == 5 and all(k.startswith("movevalue_") for k in new), new
    assert not [(k, old) for k in new for old in OLD_KERNELS + ("gamepairs_", "balance_sums_kernel", "amaf_counts") if old in k]


def resources(path, tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, path), "-o", str(tmp_path / "t.so")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]

    def fields(name):
        (block,) = [b for b in blocks if re.search(r"\d" + name + "E", b.split()[0])]
        return {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in
                (("occupancy", r"Occupancy \[waves/SIMD\]"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                 ("sspill", r"SGPRs Spill"), ("vspill", r"VGPRs Spill"), ("lds", r"LDS Size \[bytes/block\]"),
                 ("vgprs", r" VGPRs"))}

    return r.stderr, blocks, fields


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_new_kernels_keep_the_resource_conditions_beside_the_kernels_they_wrap(tmp_path):
    """Zero spills and zero scratch in every kernel of the playout translation unit; the three playout kernels at an
    occupancy of at least the tactical kernel's, itself at least 4, within 128 VGPRs, and with at most the staged table's
    324 bytes and 16 of alignment more LDS than the kernel each wraps; the two update kernels without spills or scratch."""
    err, blocks, fields = resources("bk_playout_pat.hip", tmp_path)
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", err)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)
    assert len(spills) == 2 * len(blocks) and len(scratch) == len(blocks)
    assert all(int(n) == 0 for _, n in spills) and all(int(n) == 0 for n in scratch), (spills, scratch)
    tactical = fields("tactical_playouts_kernel")
    for new, wrapped in (("movevalue_draw_kernel", "tactical_playouts_kernel"), ("movevalue_single_kernel", "reply_playouts_kernel"),
                         ("movevalue_pairs_kernel", "lgr2_playouts_kernel")):
        f, g = fields(new), fields(wrapped)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (new, f)
        assert f["occupancy"] >= tactical["occupancy"] >= 4 and f["vgprs"] <= 128, (new, f, tactical)
        assert f["lds"] <= g["lds"] + 324 + 16, (new, f, g)
    _, blocks, fields = resources("bk_playout_mast_update.hip", tmp_path)
    assert len(blocks) == 2
    for name in ("movevalue_counts_kernel", "movevalue_apply_kernel"):
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0 and f["occupancy"] >= 4, (name, f)

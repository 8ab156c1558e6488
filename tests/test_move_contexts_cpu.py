"""NAST playouts (move values keyed by the previous move) without a GPU: the update mirror against the definition
in Python integers, the three invariants of include/bokego_train.h on the host, min_plays at its edges, the previous move,
the table class, the Python surface, and what the header, the bindings and the build say."""
import copy
import ctypes
import dataclasses
import itertools
import os
import pickle
import re

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, selfplay
from bokego_amd import lockstep as L
from bokego_amd import movecontexts as MC
from bokego_amd import movevalues as MV
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS
from bokego_amd.playout_options import PlayoutOptions
from conftest import REPO
from test_amaf_cpu import seeded_tables
from test_game_pair_tables_cpu import OLD_KERNELS, kernels_of
from test_mast_cpu import HIPCC, ramp_lut, resources, same_games
from test_replies_cpu import random_histories, start
from test_reply_pairs_cpu import learned_nine, nine_records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
PASS, NONE = go.PASS, RO.MOVE_NONE
SEED = 5
SELECTORS = ("tactical_playouts_kernel", "reply_playouts_kernel", "lgr2_", "movevalue_", "gamevalues_", "gamepairs_",
             "reply_tables_", "balance_sums_kernel", "amaf_counts", "random_playouts_kernel", "pattern_playouts_kernel",
             "codes_kernel")


def index_of(played, won, k):
    return min((64 * (2 * won + k)) // (2 * (played + k)), 64)       # Python integers: exact


def definition(counts, recs, moves, won, records, playouts, lut, k, limit, min_plays):
    """The header's update, a loop over plies in Python integers -> (counts [2][82][81][2], values [2][82][81]) as lists."""
    counts = [[[list(e) for e in plane] for plane in side] for side in counts]
    for row in range(records * playouts):
        rec = recs[row // playouts]
        c0 = int(rec[L.OFF_TURN:L.OFF_TURN + 4].view(np.int32)[0]) & 1
        prev = int(rec[L.OFF_LAST_MOVE:L.OFF_LAST_MOVE + 2].view(np.int16)[0])
        for t, m in enumerate(int(x) for x in moves[row]):
            if m <= NONE:
                break
            if 0 <= m <= 80:
                mover_won = int((int(won[row]) != 0) == (t % 2 == 0))
                for p in ([81] + ([prev] if 0 <= prev <= 80 else [])):
                    e = counts[c0 ^ (t & 1)][p][m]
                    e[0] += 1
                    e[1] += mover_won
            prev = m
    for c, p, m in itertools.product(range(2), range(82), range(81)):
        e = counts[c][p][m]
        while limit > 0 and e[0] >= limit:
            e[0], e[1] = e[0] >> 1, e[1] >> 1
        assert 0 <= e[1] <= e[0]
    values = [[[0] * 81 for _ in range(82)] for _ in range(2)]
    for c, m in itertools.product(range(2), range(81)):
        i1 = index_of(*counts[c][81][m], k)
        values[c][81][m] = int(lut[i1])
        for p in range(81):
            e = counts[c][p][m]
            values[c][p][m] = int(lut[(i1 + index_of(*e, k)) >> 1]) if e[0] >= min_plays else values[c][81][m]
    return counts, values


def table_of(counts=None, k=16, limit=16384, min_plays=8, lut=None, tau=0.25):
    t = MC.MoveContextTable.empty(tau, k, limit, min_plays)
    if lut is not None:
        t = MC.MoveContextTable(t.counts, np.full((2, 82, 81), lut[32], np.uint16), lut, k, limit, min_plays)
    if counts is not None:
        t.counts[...] = counts
    return t


def seeded_counts(rng, top):
    counts = np.zeros((2, 82, 81, 2), np.int64)
    counts[..., 0] = rng.integers(0, top, (2, 82, 81))
    counts[..., 1] = rng.integers(0, 1 << 30, (2, 82, 81)) % (counts[..., 0] + 1)
    return counts


def check(table, recs, moves, won, records, playouts):
    want = definition(table.counts.tolist(), recs, moves, won, records, playouts, table.lut, table.k, table.limit, table.min_plays)
    plays = MC.move_context_update_host(table, recs, moves, won, records, playouts)
    assert table.counts.tolist() == want[0] and table.values.tolist() == want[1]
    assert (table.counts[..., 1] <= table.counts[..., 0]).all() and (table.counts >= 0).all() and (table.values >= 1).all()
    return plays


# ---- 1. the update ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records,playouts,max_plies", [(1, 1, 1), (2, 3, 8), (3, 5, 20)])
def test_the_mirror_equals_a_loop_over_plies(records, playouts, max_plies):
    recs, moves, won = random_histories(records, playouts, max_plies, 7 * records + max_plies)
    for k, limit, min_plays in ((1, 0, 1), (65536, 2, 1), (16, 16384, 8), (16, 16, 16), (3, 4, 2)):
        rng = np.random.default_rng(k + limit)
        for counts in (None, seeded_counts(rng, max(4 * limit, 50))):
            t = table_of(counts, k, limit, min_plays, ramp_lut())
            check(t, recs, moves, won, records, playouts)
            check(t, recs, moves, won, records, playouts)             # and once more on what that left


def test_the_previous_move_a_pass_the_records_last_move_and_a_record_without_one():
    recs = np.stack([start(40, 0), start(PASS, 1), start(go._NO_MOVE, 0), start(300, 0)])
    moves = np.array([[41, 42, PASS, 43, 90, 44, NONE, 45],          # after 40; 43 follows a pass; 44 follows junk
                      [13, NONE, NONE, NONE, NONE, NONE, NONE, NONE],   # the record's last move is a pass; white moves
                      [5, 6, NONE, NONE, NONE, NONE, NONE, NONE],     # a record without a last move
                      [7, 7, NONE, NONE, NONE, NONE, NONE, NONE]], np.int16)   # junk in the record; 7 after 7
    won = np.array([1, 0, 1, 1], np.uint8)
    t = table_of(k=1, limit=0, min_plays=1, lut=ramp_lut())
    assert check(t, recs, moves, won, 4, 1) == 4 + 1 + 2 + 2
    c = t.counts
    assert c[0, 40, 41].tolist() == [1, 1] and c[1, 41, 42].tolist() == [1, 0]          # ply 0: the record's last move
    assert c[1, :81, 43].sum() == 0 and c[1, 81, 43].tolist() == [1, 0]                 # after a pass: plane 81 alone
    assert c[1, :81, 44].sum() == 0 and c[1, 81, 44].tolist() == [1, 0]                 # after an entry above 80
    assert c[:, :, 45].sum() == 0                                                       # behind the end
    assert c[1, :81, 13].sum() == 0 and c[1, 81, 13].tolist() == [1, 0]                 # white moved first and lost: won == 0
    assert c[0, :81, 5].sum() == 0 and c[1, 5, 6].tolist() == [1, 0]
    assert c[0, :81, 7].sum() == 0 and c[1, 7, 7].tolist() == [1, 0] and c[0, 81, 7].tolist() == [1, 1]
    assert int(c[:, 81, :, 0].sum()) == 9 and int(c[:, :81, :, 0].sum()) == 4
    lut = ramp_lut()
    assert t.values[0, 40, 41] == lut[(index_of(1, 1, 1) + index_of(1, 1, 1)) >> 1] and t.values[0, 3, 41] == t.values[0, 81, 41]
    assert np.array_equal(MC.context_of([PASS, NONE, -100, 0, 80, 81, 300, go._NO_MOVE]), [81, 81, 81, 0, 80, 81, 81, 81])


def test_min_plays_at_its_edges_and_after_the_shift():
    lut = ramp_lut()
    recs, moves, won = np.stack([start(40, 0)]), np.full((1, 2), NONE, np.int16), np.zeros(1, np.uint8)   # nothing is added
    counts = np.zeros((2, 82, 81, 2), np.int64)
    counts[0, 81, 9] = (40, 10)
    counts[0, 1, 9], counts[0, 2, 9] = (7, 7), (8, 8)                 # min_plays - 1 and min_plays
    counts[0, 3, 9] = (17, 17)                                        # limit 16: shifted once to (8, 8), still counts
    counts[0, 4, 9] = (30, 30)                                        # ... and to (15, 15)
    t = table_of(counts, k=1, limit=0, min_plays=8, lut=lut)
    check(t, recs, moves, won, 1, 1)
    i1 = index_of(40, 10, 1)
    assert t.values[0, 81, 9] == lut[i1] and t.values[0, 1, 9] == lut[i1] and t.values[0, 2, 9] == lut[(i1 + index_of(8, 8, 1)) >> 1]
    assert t.values[0, 2, 9] != t.values[0, 1, 9]
    t = table_of(counts, k=1, limit=16, min_plays=8, lut=lut)
    check(t, recs, moves, won, 1, 1)
    assert t.counts[0, 81, 9].tolist() == [10, 2] and t.counts[0, 3, 9].tolist() == [8, 8] and t.counts[0, 4, 9].tolist() == [15, 15]
    i1 = index_of(10, 2, 1)
    assert t.values[0, 3, 9] == lut[(i1 + index_of(8, 8, 1)) >> 1] and t.values[0, 1, 9] == lut[i1]
    t = table_of(counts, k=1, limit=16, min_plays=9, lut=lut)         # the shift takes (17, 17) back below min_plays
    check(t, recs, moves, won, 1, 1)
    assert t.values[0, 3, 9] == lut[i1] and t.values[0, 4, 9] == lut[(i1 + index_of(15, 15, 1)) >> 1]
    t = table_of(counts, k=1, limit=16, min_plays=16, lut=lut)        # min_plays >= limit: no context ever qualifies
    check(t, recs, moves, won, 1, 1)
    assert (t.values[:, :81] == t.values[:, 81:82]).all()


# ---- 2. the invariants -----------------------------------------------------------------------------------------------------------
def test_plane_81_is_the_move_value_update():
    recs, moves, won = random_histories(3, 5, 20, 7)
    for k, limit, min_plays in ((1, 0, 1), (16, 16384, 8), (3, 4, 2)):
        c = table_of(seeded_counts(np.random.default_rng(k), max(4 * limit, 50)), k, limit, min_plays, ramp_lut())
        v = c.move_values()
        for _ in range(2):
            a = MC.move_context_update_host(c, recs, moves, won, 3, 5)
            b = MV.move_value_update_host(v, recs, moves, won, 3, 5)
            assert a == b and np.array_equal(c.counts[:, 81], v.counts) and np.array_equal(c.values[:, 81], v.values)
        got = c.move_values()
        assert type(got) is MV.MoveValueTable and np.array_equal(got.counts, v.counts) and (got.k, got.limit) == (k, limit)


def learned_contexts(min_plays=1, limit=0, seed=3):
    """A table with learned counts and a sharp lut, so that the games differ: 8 uniform playouts of the nine records."""
    t = MC.MoveContextTable.empty(tau=0.05, k=1, limit=limit, min_plays=min_plays)
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
        t = MC.MoveContextTable.empty()
        valued = RO.random_playouts(recs, SEED, rules="host", replies=r2, move_values=t, **kw)
        assert same_games(plain, valued) and t.occupancy() > 200, list(kw)
        assert r1 is None or np.array_equal(r1.array, r2.array)
        want = MC.MoveContextTable.empty()
        MC.move_context_update_host(want, recs, plain.moves, (plain.score > 0) == L.black_to_move(recs), 9, 1)
        assert np.array_equal(t.counts, want.counts) and np.array_equal(t.values, want.values)
    learned = learned_contexts()
    assert learned.values[:, :81].min() < 100 and learned.values[:, :81].max() > 600 and learned.qualified() > 100
    assert (learned.values[:, :81] != learned.values[:, 81:82]).any()
    a, b = (RO.random_playouts(recs, SEED, rules="host", patterns=pat, tactics=tac, move_values=learned.copy()) for _ in range(2))
    assert same_games(a, b) and not same_games(a, RO.random_playouts(recs, SEED, rules="host", patterns=pat, tactics=tac))
    assert not same_games(a, RO.random_playouts(recs, SEED, rules="host", patterns=pat, tactics=tac, move_values=learned.move_values()))
    v = [RO.playout_value(recs, 4, SEED, rules="host", move_values=t) for t in (learned.copy(), learned.copy(), None)]
    assert np.array_equal(v[0], v[1]) and not np.array_equal(v[0], v[2])
    am = RO.playout_amaf(recs, 4, SEED, rules="host", move_values=learned.copy(), sides=2)
    assert np.array_equal(am.value, v[0]) and am.played.shape == (9, 2, 81)


def test_with_min_plays_at_the_limit_the_games_are_the_move_value_games():
    recs = nine_records()
    pat, tac = seeded_tables()
    c = MC.MoveContextTable.empty(tau=0.05, k=1, limit=64, min_plays=64)
    v = MV.MoveValueTable.empty(tau=0.05, k=1, limit=64)
    for kw in (dict(), dict(patterns=pat, tactics=tac), dict(replies=RO.ReplyTable2.empty)):
        make = kw.pop("replies", None)
        for _ in range(2):                                            # the second round draws with what the first one learned
            r1, r2 = (None, None) if make is None else (make(), make())
            a = RO.playout_value(recs, 4, SEED, rules="host", move_values=c, replies=r1, **kw)
            b = RO.playout_value(recs, 4, SEED, rules="host", move_values=v, replies=r2, **kw)
            assert np.array_equal(a, b)
            x = RO.random_playouts(recs, SEED, rules="host", move_values=c, replies=r1, **kw)
            y = RO.random_playouts(recs, SEED, rules="host", move_values=v, replies=r2, **kw)
            assert same_games(x, y)
            assert np.array_equal(c.counts[:, 81], v.counts) and np.array_equal(c.values[:, 81], v.values)
            assert (c.values[:, :81] == c.values[:, 81:82]).all() and c.counts[:, :81, :, 0].max() < 64
    assert (v.values != 256).any() and c.qualified() == 0
    # _random_host itself, as the definition names it: the same table read two ways
    ctr = RO.default_counters(9, RO.record_turns(recs))
    a = RO._random_host(recs, L.seed_u64(SEED), ctr, 400, L.KOMI, True, move_values=c)
    b = RO._random_host(recs, L.seed_u64(SEED), ctr, 400, L.KOMI, True, move_values=c.move_values())
    assert same_games(a, b)


def test_the_weight_rule_indexes_colour_previous_move_and_point():
    values = (np.arange(2 * 82 * 81) % 60000 + 1).astype(np.uint16).reshape(2, 82, 81)   # every entry its own value
    w = np.full((6, 81), 512, np.int64)
    colour, prev = np.array([0, 1, 0, 1, 0, 1]), np.array([0, 80, PASS, NONE, 300, 40])
    got = MC.move_context_weights(w, values, colour, prev)
    for r, (c, p) in enumerate(zip(colour.tolist(), [0, 80, 81, 81, 81, 40])):
        assert got[r].tolist() == [(512 * int(values[c, p, q])) >> 8 for q in range(81)]
    neutral = np.full((2, 82, 81), 256, np.uint16)
    assert np.array_equal(MC.move_context_weights(w, neutral, colour, prev), w.astype(np.uint64))
    assert (MC.move_context_weights(np.full((6, 81), 1 << 23), np.full((2, 82, 81), 65535, np.uint16), colour, prev) == (1 << 24) - 1).all()
    assert (MC.move_context_weights(np.full((6, 81), 255), np.full((2, 82, 81), 1, np.uint16), colour, prev) == 1).all()
    t = MC.MoveContextTable(np.zeros((2, 82, 81, 2), np.int64), values, MV.lut_of(1.0))
    assert np.array_equal(MC.move_context_weights(w, t, colour, prev), got)
    for bad in (values.astype(np.int16), values[:, 81], values[:, :81]):
        with pytest.raises(ValueError):
            MC.move_context_weights(w, bad, colour, prev)


# ---- 3. the table class ----------------------------------------------------------------------------------------------------------
def test_the_table_class_copies_clears_and_pickles():
    t = learned_contexts(min_plays=3)
    assert (t.k, t.limit, t.min_plays) == (1, 0, 3) and t.occupancy() > 300 and np.array_equal(t.lut, MV.lut_of(0.05))
    assert t.counts.shape == (2, 82, 81, 2) and t.counts.dtype == np.int64 and t.values.shape == (2, 82, 81) and t.values.dtype == np.uint16
    assert (t.counts[..., 1] <= t.counts[..., 0]).all() and (t.counts[:, :81, :, 0].sum(1) <= t.counts[:, 81, :, 0]).all()
    for other in (t.copy(), copy.deepcopy(t), pickle.loads(pickle.dumps(t)), copy.deepcopy({"x": t})["x"]):
        assert other is not t and type(other) is MC.MoveContextTable and (other.k, other.limit, other.min_plays) == (1, 0, 3)
        assert all(np.array_equal(getattr(other, f), getattr(t, f)) for f in ("counts", "values", "lut"))
        other.counts[0, 0, 0, 0] += 1
        assert other.counts[0, 0, 0, 0] == t.counts[0, 0, 0, 0] + 1
    u = t.copy()
    u.clear()
    assert not u.counts.any() and (u.values == 256).all() and u.occupancy() == 0 and u.qualified() == 0 and t.occupancy() > 300
    e = MC.MoveContextTable.empty()
    assert (e.k, e.limit, e.min_plays) == (16, 16384, 8) == (MV.DEFAULT_K, MV.DEFAULT_LIMIT, MC.DEFAULT_MIN_PLAYS)
    assert np.array_equal(e.lut, MV.lut_of(MV.DEFAULT_TAU)) and not e.counts.any() and (e.values == 256).all()
    zeros, neutral, lut = np.zeros((2, 82, 81, 2), np.int64), np.full((2, 82, 81), 256, np.uint16), MV.lut_of(1.0)
    for bad in (dict(counts=zeros.astype(np.int32)), dict(counts=zeros[:, 81]), dict(values=neutral.astype(np.int16)),
                dict(values=neutral[:, 81]), dict(values=np.zeros((2, 82, 81), np.uint16)), dict(lut=lut[:64]), dict(k=0),
                dict(limit=1), dict(min_plays=0), dict(min_plays=(1 << 30) + 1), dict(counts=zeros - 1),
                dict(counts=zeros + np.array([1, 2]))):
        with pytest.raises(ValueError):
            MC.MoveContextTable(**{**dict(counts=zeros, values=neutral, lut=lut, k=1, limit=0, min_plays=1), **bad})
    with pytest.raises(TypeError):
        MC.MoveContextTable(zeros, neutral, lut, 1, 0, 2.5)
    assert MC.MoveContextTable(zeros, neutral, lut, 1, 0, 1 << 30).min_plays == 1 << 30 == MC.MAX_MIN_PLAYS
    recs, moves, won = random_histories(2, 3, 8, 1)
    for args in ((recs, moves, won, 3, 2), (recs, moves, won, 0, 6), (recs, moves[:5], won[:5], 2, 3), (recs[:1], moves, won, 2, 3),
                 (recs, np.zeros((6, 1025), np.int16), won, 2, 3)):
        with pytest.raises(ValueError):
            MC.move_context_update_host(e, *args)
    for not_a_context_table in (MV.MoveValueTable.empty(), e.values):
        with pytest.raises(TypeError):
            MC.move_context_update_host(not_a_context_table, recs, moves, won, 2, 3)
    assert e.occupancy() == 0


# ---- 4. the refusals, the evaluator, the options, the front ends -------------------------------------------------------------------
def test_the_refusals_of_the_playout_functions():
    recs = nine_records()[:3]
    t = MC.MoveContextTable.empty()
    with pytest.raises(ValueError, match="move-value"):
        RO.playout_ownership(recs, 2, SEED, rules="host", move_values=t)
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", slots=np.array([0, 1, 0]), move_values=t)
    for per_game in (RO.ReplyTables(2), RO.ReplyTables2(2)):
        with pytest.raises(TypeError, match="slots"):
            RO.random_playouts(recs, SEED, rules="host", replies=per_game, slots=np.array([0, 1, 0]), move_values=t)
        with pytest.raises((TypeError, ValueError)):
            RO.random_playouts(recs, SEED, rules="host", replies=per_game, move_values=t)
    assert t.occupancy() == 0


def test_the_evaluator_keeps_a_table_and_its_first_request_is_the_plain_one():
    recs = nine_records()[[1, 3, 4]]
    same = lambda x: x                                                # noqa: E731
    for more in (dict(), dict(replies=True), dict(replies=2, rave=True)):
        plain = RO.PlayoutEvaluator(None, 4, seed=SEED, rules="host", prior=1.0, **more)
        ev = RO.PlayoutEvaluator(None, 4, seed=SEED, rules="host", prior=1.0, move_contexts=True, **more)
        assert type(ev.move_values) is MC.MoveContextTable and ev.move_values.occupancy() == 0 and not ev.wants_games
        a, b = plain.finish(plain.submit(recs, 1), normalise=same), ev.finish(ev.submit(recs, 1), normalise=same)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[:2], b[:2])) and ev.move_values.occupancy() > 100
        plays = int(ev.move_values.counts[:, 81, :, 0].sum())
        ev.finish(ev.submit(recs, 1), normalise=same)
        assert int(ev.move_values.counts[:, 81, :, 0].sum()) > plays and not (ev.move_values.values == 256).all()
        ev.reset_move_values()
        assert ev.move_values.occupancy() == 0 and (ev.move_values.values == 256).all()
    ev = RO.PlayoutEvaluator(None, 4, seed=SEED, rules="host", prior=1.0, move_contexts=0.1)
    t = ev.move_values
    assert np.array_equal(t.lut, MV.lut_of(0.1)) and (t.k, t.limit, t.min_plays) == (16, 16384, 8)
    for bad in (dict(move_values=True), dict(move_values=0.5), dict(replies=True, games=2), dict(pair_games=2), dict(move_value_games=2)):
        with pytest.raises(TypeError, match="move_contexts"):
            RO.PlayoutEvaluator(None, 4, rules="host", prior=1.0, move_contexts=True, **bad)
    with pytest.raises(ValueError, match="tau"):
        RO.PlayoutEvaluator(None, 4, rules="host", prior=1.0, move_contexts=-0.5)
    assert RO.PlayoutEvaluator(None, 4, rules="host", prior=1.0, move_contexts=False).move_values is None


def test_the_option_and_the_command_lines(capsys):
    assert PlayoutOptions(2, 3, "host").playout_move_contexts == 0.0 and "playout_move_contexts" not in vars(PlayoutOptions())
    with pytest.raises(TypeError):
        PlayoutOptions(playout_value=8, playout_move_contexts=0.25)
    names = [f.name for f in dataclasses.fields(PlayoutOptions)]
    assert names[-4:] == ["playout_move_contexts", "playout_move_values", "playout_reply_pairs", "playout_replies"]
    o = PlayoutOptions(playout_value=8)
    o.playout_move_contexts = 0.5
    assert o == PlayoutOptions.from_keywords(dict(playout_value=8, playout_move_contexts=0.5)) and o != PlayoutOptions(playout_value=8)
    assert o.search_keywords() == dict(playout_value=8, playout_move_contexts=0.5)
    assert o.evaluator_keywords() == dict(playouts=8, seed=0, rules="device", move_contexts=0.5) and o.name_suffix() == "-mc8-nast"
    both = PlayoutOptions.from_keywords(dict(playout_value=8, playout_reply_pairs=True, playout_move_contexts=0.25, playout_rave=4))
    assert both.evaluator_keywords() == dict(playouts=8, seed=0, rules="device", rave=True, replies=2, move_contexts=0.25)
    assert both.name_suffix() == "-mc8-rave4-lgr2-nast"
    off = PlayoutOptions.from_keywords(dict(playout_value=8, playout_reply_pairs=True, playout_move_values=0.25, playout_rave=4))
    assert off.name_suffix() == "-mc8-rave4-lgr2-mast" and "move_contexts" not in off.evaluator_keywords()
    assert "playout_move_contexts" not in off.search_keywords() and PlayoutOptions.from_keywords(dict(playout_value=8)).name_suffix() == "-mc8"
    with pytest.raises(TypeError, match="playout_move_contexts.*playout_value"):
        PlayoutOptions.from_keywords(dict(playout_move_contexts=0.25))
    with pytest.raises(TypeError, match="playout_move_contexts.*playout_move_values"):
        PlayoutOptions.from_keywords(dict(playout_value=8, playout_move_contexts=0.25, playout_move_values=0.25))
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="playout_move_contexts"):
            PlayoutOptions.from_keywords(dict(playout_value=8, playout_move_contexts=bad))
    for mod in (gtp, match):
        a = mod.parse_args(["--playout-value", "8", "--playout-prior", "1", "--playout-move-contexts"])
        assert a.playout.playout_move_contexts == 0.25 and a.playout.name_suffix().endswith("-nast")
        a = mod.parse_args(["--playout-value", "8", "--playout-prior", "1", "--playout-move-contexts", "0.1", "--playout-reply-pairs"])
        assert a.playout.evaluator_keywords()["move_contexts"] == 0.1 and a.playout.evaluator_keywords()["replies"] == 2
        assert mod.parse_args(["--playout-value", "8", "--playout-prior", "1"]).playout.playout_move_contexts == 0.0
        for argv, named in ((["--playout-move-contexts"], "--playout-value"),
                            (["--playout-value", "8", "--playout-move-contexts", "-1"], "--playout-move-contexts"),
                            (["--playout-value", "8", "--playout-move-contexts", "nan"], "--playout-move-contexts"),
                            (["--playout-value", "8", "--playout-move-contexts", "--playout-move-values"], "--playout-move-values")):
            with pytest.raises(SystemExit):
                mod.parse_args(argv)
            err = capsys.readouterr().err
            assert named in err and "--playout-move-contexts" in err
    with pytest.raises(SystemExit):                                   # one evaluator serves many games there
        selfplay.parse_args(["--playout-value", "8", "--playout-move-contexts"])
    assert "--playout-move-contexts" in capsys.readouterr().err and not hasattr(selfplay.parse_args([]), "playout_move_contexts")
    import argparse
    ap = argparse.ArgumentParser()
    PlayoutOptions.add_arguments(ap)
    text = " ".join(ap.format_help().split())
    assert "--playout-move-contexts [TAU]" in text and "untuned" in text.split("--playout-move-contexts [TAU]")[-1].split("--playout-move-values [TAU]")[0]
    a = RO._parse(["--sgf", "g.sgf", "--random", "--move-contexts", "-n", "64", "--chunk", "8"])
    assert a.move_contexts is True and a.chunk == 8 and RO._parse(["--sgf", "g.sgf", "--random"]).move_contexts is False
    for bad in (["--move-contexts"], ["--random", "--move-contexts", "--amaf"], ["--random", "--move-contexts", "--replies"],
                ["--random", "--move-contexts", "--move-values"], ["--random", "--move-contexts", "--chunk", "0"]):
        with pytest.raises(SystemExit):
            RO._parse(["--sgf", "g.sgf"] + bad)
    capsys.readouterr()
    rep = RO.move_contexts_report(nine_records()[1:2], 16, SEED, 4, rules="host")
    assert rep["playouts"] == 16 and 0 < rep["played_share"] <= 1 and 0 <= rep["context_qualified_share"] <= rep["context_played_share"] and 0 < rep["context_played_share"] < 1
    assert rep["min_value"] < 256 < rep["max_value"] and len(rep["heaviest"]) == 10 and rep["min_plays"] == 8
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "--playout-move-contexts" in readme and "## 32." in open(os.path.join(REPO, "DESIGN.md")).read()


def test_native_mcts_and_gtp_keep_the_table_with_the_search():
    from bokego_amd.mcts_native import Position
    seen = []
    for _ in range(2):
        t = NativeMCTS(None, None, None, playout_value=2, playout_prior=1, playout_rules="host", playout_move_contexts=0.25,
                       playout_replies=True, playout_seed=SEED)
        assert t.playout_move_contexts == 0.25 and type(t.evaluator.move_values) is MC.MoveContextTable
        t.rollout(12)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.evaluator.move_values.counts.copy()))
        twin = copy.deepcopy(t)
        assert twin.evaluator is not t.evaluator and twin.evaluator.move_values.occupancy() == 0
        twin.close()
        t.close()
    assert seen[0][0] == seen[1][0] and np.array_equal(seen[0][1], seen[1][1]) and seen[0][1][:, :81].any()
    t = NativeMCTS(None, None, None, playout_value=2, playout_prior=1, playout_rules="host")
    assert t.playout_move_contexts == 0.0 and t.evaluator.move_values is None
    t.close()
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(None, None, None, playout_move_contexts=0.25, playout_prior=1)
    with pytest.raises(TypeError, match="playout_move_values"):
        NativeMCTS(None, None, None, playout_value=2, playout_prior=1, playout_move_contexts=0.25, playout_move_values=0.25)
    g = gtp.NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=4, playout_value=2, playout_prior=1,
                      playout_move_contexts=0.25, playout_rules="host")
    try:
        g.running = True
        assert g.send("genmove b").startswith("= ") and g.evaluator.move_values.occupancy() > 0
        assert g.send("clear_board") == "= \n\n" and g.evaluator.move_values.occupancy() == 0
        assert g.send("genmove b").startswith("= ")
    finally:
        g.close()


# ---- 5. header, bindings, build ---------------------------------------------------------------------------------------------------
def test_header_bindings_makefile_and_the_kernels_names():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_MOVE_CONTEXT_MAX_MIN_PLAYS\s+\(1 << 30\)", src)
    assert T.MOVE_CONTEXT_MAX_MIN_PLAYS == 1 << 30 == MC.MAX_MIN_PLAYS
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_move_context_playouts\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*const\s+uint16_t\s*\*\s*values\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*replies\s*,\s*const\s+uint8_t\s*\*\s*replies2\s*,\s*int\s+max_plies\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,"
                     r"\s*int32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bsize_t\s+bkt_move_context_scratch_bytes\s*\(\s*int\s+records\s*\)", code)
    assert re.search(r"\bint\s+bkt_move_context_update\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*const\s+int16_t\s*\*\s*moves\s*,"
                     r"\s*int\s+max_plies\s*,\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*int64_t\s*\*\s*counts\s*,\s*uint16_t\s*\*\s*values\s*,\s*const\s+uint16_t\s*\*\s*lut\s*,\s*int\s+k\s*,"
                     r"\s*int\s+limit\s*,\s*int\s+min_plays\s*,\s*void\s*\*\s*scratch\s*,\s*void\s*\*\s*stream\s*\)", code)
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("counts int64 [2][82][81][2]", "values uint16 [2][82][81]", "Anything outside 0..80 (a pass, none, junk) is p = 81",
                   "w = min(2^24 - 1, max(1, ((uint64_t)w_in * values[c][p][q]) >> 8))", "reads exactly one uint16 of values per ply",
                   "counts[c][81][m] += (1, mover won) always", "counts[c][p][m] += (1, mover won) when p < 81",
                   "values[c][p][m] = lut[(i1 + i2) >> 1]", "Every entry of values is written", "No wrap.", "212,544 bytes",
                   "with min_plays >= limit > 0 no context ever qualifies", "a refused call launches nothing and writes nothing"):
        assert " ".join(phrase.replace("*", " ").split()) in flat, phrase
    P, I, U64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t
    assert T.SYMBOLS["bkt_move_context_playouts"] == (I, [P, I, U64, P, P, P, P, P, P, I, P, P, P, P, P]) and callable(T.move_context_playouts)
    assert T.SYMBOLS["bkt_move_context_update"] == (I, [P, P, I, P, I, I, P, P, P, I, I, I, P, P]) and callable(T.move_context_update)
    assert T.SYMBOLS["bkt_move_context_scratch_bytes"] == (Z, [I]) and callable(T.move_context_scratch_bytes)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        lib.bkt_move_context_scratch_bytes.restype, lib.bkt_move_context_scratch_bytes.argtypes = Z, [I]
        assert lib.bkt_abi_version() == 4 and lib.bkt_move_context_playouts and lib.bkt_move_context_update
        assert [lib.bkt_move_context_scratch_bytes(n) for n in (-1, 0, 1, 3, 1024)] == [0, 0, 212544, 212544, 212544]
    make = open(os.path.join(CSRC, "Makefile")).read()
    rule, line = re.search(r"^\$\(TRAIN_OUT\):(.*)\n\t(.*)$", make, flags=re.M).groups()
    assert "bk_playout_nast.hip" in rule.split() and "bk_playout_nast.hip" not in line.split()
    assert "bk_playout_nast_update.hip" in rule.split() and "bk_playout_nast_update.hip" in line.split("-shared")[0].split()
    assert "-shared bk_train.hip bk_train_bf16.hip bk_playout_pat.hip -o" in line
    assert "bk_playout_mast_update.hip bk_playout_mast_tables_update.hip" in rule and "bk_playout_mast_update.hip bk_playout_mast_tables_update.hip" in line
    # included as text at the very end of bk_playout_reply2.hip, behind its entry points: the pinned includes stay
    host = open(os.path.join(CSRC, "bk_playout_reply2.hip")).read()
    assert re.findall(r'^#include "([^"]+)"', host, flags=re.M) == ["bk_playout_nast.hip"]
    last = host.rstrip().splitlines()[-1]
    assert last.startswith('#include "bk_playout_nast.hip"') and host.index("bkt_reply2_update(") < host.index(last)
    assert "balance" not in host and "float" not in host
    includes = re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, "bk_playout_pat.hip")).read(), flags=re.M)
    assert includes[-2:] == ["bk_playout_reply2.hip", "bk_playout_reply2_tables.hip"]
    draw, update = (open(os.path.join(CSRC, name)).read() for name in ("bk_playout_nast.hip", "bk_playout_nast_update.hip"))
    for own in (draw, update):
        assert "float" not in own and "double" not in own
    assert "__syncthreads" not in draw and "__shared__" not in draw and "#include" not in draw.split("namespace {")[0].replace("included as text", "")
    assert not re.search(r"\batomic\w*\s*\(", draw)
    assert re.findall(r"^#include\s+(\S+)", update, flags=re.M) == ["<hip/hip_runtime.h>", "<stdint.h>", '"../../include/bokego_train.h"']
    assert set(re.findall(r"\b(atomic\w*)\s*\(", update)) == {"atomicAdd"}    # integer adds only: no exchange, no max, no CAS
    for inst in ("WeightedDraw<ContextValueWeight>", "ReplyDraw<WeightedDraw<ContextValueWeight>, 1>", "Reply2Draw<WeightedDraw<ContextValueWeight>>"):
        assert inst in draw, inst
    body = draw.split("unsigned operator()")[1].split("};")[0]
    assert body.index("values[") < body.index("inner(W")              # the read is issued before the tactical weight
    new = kernels_of("bk_playout_nast.hip") + kernels_of("bk_playout_nast_update.hip")
    assert len(new) == 6 and len(set(new)) == 6 and all(k.startswith("ctxvalue_") for k in new), new
    assert not [(k, old) for k in new for old in OLD_KERNELS + SELECTORS if old in k]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_new_kernels_keep_the_resource_conditions_beside_the_kernels_they_wrap(tmp_path):
    """Zero spills and zero scratch in every kernel of the playout translation unit; the three playout kernels at an
    occupancy of at least the tactical kernel's, itself at least 4, within 128 VGPRs, and with at most 16 bytes more LDS than
    the kernel each wraps (nothing is staged); the update unit has exactly its own three kernels, without spills or scratch
    and at an occupancy of at least 4."""
    err, blocks, fields = resources("bk_playout_pat.hip", tmp_path)
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", err)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)
    assert len(spills) == 2 * len(blocks) and len(scratch) == len(blocks) and len(blocks) == 37
    assert all(int(n) == 0 for _, n in spills) and all(int(n) == 0 for n in scratch), (spills, scratch)
    tactical = fields("tactical_playouts_kernel")
    for new, wrapped in (("ctxvalue_draw_kernel", "tactical_playouts_kernel"), ("ctxvalue_single_kernel", "reply_playouts_kernel"),
                         ("ctxvalue_pairs_kernel", "lgr2_playouts_kernel")):
        f, g = fields(new), fields(wrapped)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (new, f)
        assert f["occupancy"] >= tactical["occupancy"] >= 4 and f["vgprs"] <= 128, (new, f, tactical)
        assert f["lds"] <= g["lds"] + 16, (new, f, g)
    _, blocks, fields = resources("bk_playout_nast_update.hip", tmp_path)
    assert len(blocks) == 3
    for name in ("ctxvalue_init_kernel", "ctxvalue_counts_kernel", "ctxvalue_apply_kernel"):
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0 and f["occupancy"] >= 4, (name, f)

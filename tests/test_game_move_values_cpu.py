"""A move-value table per game of a self-play batch, without a GPU: the host mirrors over many tables against
the single-table mirrors per slot, the class and what is refused, the evaluator with move_value_games=, self_play on the host
rules, the flag, and what the header, the bindings and the build say."""
import copy
import ctypes
import inspect
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import movevalues as MV
from bokego_amd import rollout as RO
from bokego_amd import selfplay
from conftest import REPO
from test_amaf_cpu import seeded_tables
from test_game_pair_tables_cpu import FORCED, OLD_KERNELS, REQUESTS, abc_tables, histories, host_counters, kernels_of, nine, padded, requests
from test_game_tables_cpu import KW, _bits
from test_mast_cpu import resources

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
SEED = 5
SLOTS = np.array([0, 1, 2, 0, 0, 2, 1, 2, 0])                         # table 3 of four is named by no row

_CACHE = {}


def learned_tables():
    """Four move-value tables with a sharp lut, learned from three requests of 8 uniform playouts of the nine records each,
    every request dealing the records to other tables: the values differ per table (a copy)."""
    if "learned" not in _CACHE:
        t = MV.MoveValueTables(4, tau=0.05, k=1, limit=0)
        for k in range(3):
            RO.playout_value(nine(), 8, SEED + k, rules="host", move_values=t, slots=(np.arange(9) + k) % 4)
        _CACHE["learned"] = t
    return _CACHE["learned"].copy()


def same_tables(a, b):
    return np.array_equal(a.counts, b.counts) and np.array_equal(a.values, b.values)


# ---- 1. the mirrors against the single-table mirrors, per slot -------------------------------------------------------------
def test_the_learned_tables_differ_and_a_slot_mix_up_would_show():
    t = learned_tables()
    assert len({t.values[i].tobytes() for i in range(4)}) == 4 and t.values.min() < 100 and t.values.max() > 600
    key, ctr = host_counters(nine())
    runs = [RO._random_host(nine(), key, ctr, 400, L.KOMI, True, move_values=t.table(i)) for i in range(3)]
    free = [i for i in range(9) if i not in FORCED]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert (padded(runs[a], 400) != padded(runs[b], 400)).any(1)[free].all(), (a, b)


def test_the_playouts_with_slots_equal_the_single_table_mirror_per_slot():
    t = learned_tables()
    pat, tac = seeded_tables()
    key, ctr = host_counters(nine())
    for kw in (dict(), dict(table=pat, tactics=tac)):
        fin = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, slots=SLOTS, move_values=t, **kw)
        for s in range(3):
            rows = np.nonzero(SLOTS == s)[0]
            one = RO._random_host(nine()[rows], key, ctr[rows], 400, L.KOMI, True, move_values=t.table(s), **kw)
            assert np.array_equal(fin.records[rows], one.records) and np.array_equal(fin.plies[rows], one.plies), s
            assert np.array_equal(fin.over[rows], one.over) and np.array_equal(padded(fin, 400)[rows], padded(one, 400)), s
        turned = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, slots=(SLOTS + 1) % 3, move_values=t, **kw)
        assert all((padded(fin, 400)[i] != padded(turned, 400)[i]).any() for i in range(9) if i not in FORCED)
    # under a pair table per game the same slot names both tables of a row
    pairs = np.concatenate([abc_tables(), abc_tables()[:1]])
    fin = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, replies=RO.ReplyTables2(4, pairs), slots=SLOTS, move_values=t)
    for s in range(3):
        rows = np.nonzero(SLOTS == s)[0]
        one = RO._random_host(nine()[rows], key, ctr[rows], 400, L.KOMI, True, replies=RO.ReplyTable2(pairs[s]), move_values=t.table(s))
        assert np.array_equal(fin.records[rows], one.records) and np.array_equal(padded(fin, 400)[rows], padded(one, 400)), s
    assert fin.reply_pair_plies > 0
    # the weight rule itself, row by row
    w = np.random.default_rng(1).integers(1, 1 << 24, (5, 81))
    slots, colour = np.array([2, 0, 2, 1, 7]), np.array([0, 1, 1, 0, 1])
    got = MV.move_value_weights(w, t, colour, slots=slots)
    for r in range(4):
        assert np.array_equal(got[r], MV.move_value_weights(w[r:r + 1], t.table(slots[r]), colour[r:r + 1])[0]), r
    assert np.array_equal(got[4], MV.move_value_weights(w[4:], np.full((2, 81), 256, np.uint16), colour[4:])[0])
    assert np.array_equal(MV.move_value_weights(w, t.values, colour, slots=slots), got)     # raw arrays are taken as the class is


def test_the_update_with_slots_equals_the_single_table_mirror_per_slot():
    recs = np.ascontiguousarray(nine()[[1, 2, 3, 4, 5]])
    slots = np.array([2, 0, 2, 1, 2])                                 # non-adjacent records of table 2
    moves, won = histories(recs, 3)
    for k, limit in ((1, 0), (16, 16384), (3, 4)):
        before = learned_tables()
        before.k, before.limit = k, limit
        before.counts[3, 0, 0] = (1 << 20, 7)                         # table 3, named by no record: played >= limit, and values
        before.values[3] = 1234                                       # that are not what its counts imply
        got = before.copy()
        plays = MV.move_value_update_host(got, recs, moves, won, 5, 3, slots=slots)
        total = 0
        for s in range(3):
            rows = np.nonzero(slots == s)[0]
            pick = (rows[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)
            want = before.table(s)
            total += MV.move_value_update_host(want, recs[rows], moves[pick], won[pick], len(rows), 3)
            assert np.array_equal(got.counts[s], want.counts) and np.array_equal(got.values[s], want.values), (k, limit, s)
            assert not np.array_equal(got.counts[s], before.counts[s]), s
        assert plays == total > 0
        assert np.array_equal(got.counts[3], before.counts[3]) and (got.values[3] == 1234).all()     # every byte is kept
        assert got.counts[3, 0, 0, 0] == 1 << 20


def test_slots_out_of_range_play_neutrally_and_update_nothing():
    t = learned_tables()
    key, ctr = host_counters(nine())
    out = np.array([-1, 4, -1, 4, 1 << 20, -(1 << 20), 4, -1, 4])     # -1, count and +-2^20
    fin = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, slots=out, move_values=t)
    plain = RO._random_host(nine(), key, ctr, 400, L.KOMI, True)
    assert np.array_equal(fin.moves, plain.moves) and np.array_equal(fin.records, plain.records)
    moves, won = histories(nine(), 2)
    got = t.copy()
    assert MV.move_value_update_host(got, nine(), moves, won, 9, 2, slots=out) == 0 and same_tables(got, t)
    mixed = np.where(np.arange(9) % 2 == 0, 1, out)                   # the records in range still count
    assert MV.move_value_update_host(got, nine(), moves, won, 9, 2, slots=mixed) > 0
    assert not np.array_equal(got.counts[1], t.counts[1])
    for i in (0, 2, 3):
        assert np.array_equal(got.counts[i], t.counts[i]) and np.array_equal(got.values[i], t.values[i]), i


def test_one_table_with_all_slots_zero_is_the_single_table_bit_for_bit():
    recs = nine()[[1, 3, 5]]
    pat, tac = seeded_tables()
    for make_one, make_many in ((lambda: None, lambda: None), (RO.ReplyTable.empty, lambda: RO.ReplyTables(1)),
                                (RO.ReplyTable2.empty, lambda: RO.ReplyTables2(1))):
        one, many = MV.MoveValueTable.empty(tau=0.1, k=2, limit=16), MV.MoveValueTables(1, tau=0.1, k=2, limit=16)
        r_one, r_many = make_one(), make_many()
        for batch in range(2):
            a = RO.playout_amaf(recs, 3, SEED, rules="host", sides=2, patterns=pat, tactics=tac, replies=r_one, move_values=one)
            b = RO.playout_amaf(recs, 3, SEED, rules="host", sides=2, patterns=pat, tactics=tac, replies=r_many, move_values=many,
                                slots=np.zeros(3, np.int64))
            for name in ("value", "wins", "played", "won"):
                assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), (batch, name)
            assert np.array_equal(many.counts[0], one.counts) and np.array_equal(many.values[0], one.values), batch
            assert r_one is None or np.array_equal(r_many.array[0], r_one.array), batch
        f1 = RO.random_playouts(recs, SEED, rules="host", replies=r_one, move_values=one)
        f2 = RO.random_playouts(recs, SEED, rules="host", replies=r_many, move_values=many, slots=[0, 0, 0])
        assert np.array_equal(f1.moves, f2.moves) and np.array_equal(many.counts[0], one.counts)
        assert np.array_equal(RO.playout_value(recs, 2, SEED, rules="host", replies=r_one, move_values=one),
                              RO.playout_value(recs, 2, SEED, rules="host", replies=r_many, move_values=many, slots=np.zeros(3, np.int32)))
        assert one.counts[..., 0].max() < 16 and one.occupancy() > 50 and same_tables(many.table(0), one)


# ---- 2. the class and what is refused ---------------------------------------------------------------------------------------
def test_the_tables_class_and_what_is_refused():
    t = MV.MoveValueTables(3, tau=0.1, k=2, limit=64)
    assert t.count == 3 and t.counts.shape == (3, 2, 81, 2) and t.counts.dtype == np.int64 and not t.counts.any()
    assert t.values.shape == (3, 2, 81) and t.values.dtype == np.uint16 and (t.values == 256).all()
    assert (t.k, t.limit) == (2, 64) and np.array_equal(t.lut, MV.lut_of(0.1)) and not t.lut.flags.writeable
    d = MV.MoveValueTables(2)
    assert (d.k, d.limit) == (MV.DEFAULT_K, MV.DEFAULT_LIMIT) and np.array_equal(d.lut, MV.lut_of(MV.DEFAULT_TAU))
    assert "MoveValueTables" in MV.__all__ and MV.MAX_TABLES == 4096 == T.MAX_MOVE_VALUE_TABLES
    t.counts[1, 0, 4], t.values[1, 0, 4], t.values[2, 1, 80] = (5, 3), 700, 9
    assert isinstance(t, MV.MoveValueTable) and t.occupancy().tolist() == [0, 1, 0]
    one = t.table(1)
    assert type(one) is MV.MoveValueTable and one.counts[0, 4].tolist() == [5, 3] and one.values[0, 4] == 700
    assert (one.k, one.limit) == (2, 64) and np.array_equal(one.lut, t.lut)
    one.counts[0, 4, 0] = 9                                           # a copy
    assert t.counts[1, 0, 4, 0] == 5 and t.copy().values[2, 1, 80] == 9 and t.copy().count == 3
    for other in (copy.deepcopy(t), pickle.loads(pickle.dumps(t)), t.copy()):
        assert type(other) is MV.MoveValueTables and other.count == 3 and same_tables(other, t)
        assert (other.k, other.limit) == (2, 64) and np.array_equal(other.lut, t.lut)
        other.counts[0, 0, 0, 0] = 1
    assert t.counts[0, 0, 0, 0] == 0
    t.clear()
    assert not t.counts.any() and (t.values == 256).all()
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError):
            MV.MoveValueTables(bad)
    assert MV.MoveValueTables(4096).count == 4096 and MV.MoveValueTables.empty(2, tau=0.1).values.shape == (2, 2, 81)
    with pytest.raises(IndexError):
        t.table(3)
    for kw in (dict(tau=0.0), dict(k=0), dict(limit=1)):
        with pytest.raises(ValueError):
            MV.MoveValueTables(2, **kw)
    recs = nine()[:3]
    many, slots = MV.MoveValueTables(2), np.array([0, 1, 0])
    with pytest.raises(TypeError, match="slots"):                     # tables per game need slots
        RO.playout_value(recs, 2, SEED, rules="host", move_values=many)
    with pytest.raises(TypeError, match="slots"):
        RO.random_playouts(recs, SEED, rules="host", move_values=many, replies=RO.ReplyTables(2))
    for single in (RO.ReplyTable.empty(), RO.ReplyTable2.empty()):    # not with one reply table for all rows
        with pytest.raises(TypeError, match="single"):
            RO.playout_value(recs, 2, SEED, rules="host", move_values=many, replies=single, slots=slots)
    for other in (RO.ReplyTables(3), RO.ReplyTables2(3)):             # equally many
        with pytest.raises(ValueError, match="equally many"):
            RO.playout_amaf(recs, 2, SEED, rules="host", move_values=many, replies=other, slots=slots)
    with pytest.raises(TypeError, match="slots"):                     # a single table with slots stays what it is
        RO.playout_value(recs, 2, SEED, rules="host", move_values=MV.MoveValueTable.empty(), replies=RO.ReplyTables(2), slots=slots)
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", move_values=MV.MoveValueTable.empty(), slots=slots)
    with pytest.raises(TypeError, match="slots"):                     # (playout_ownership launches no score and takes no slots)
        RO.playout_ownership(recs, 2, SEED, rules="host", move_values=many)
    for bad in ([0, 0], [0.0, 0.0, 0.0], [[0, 0, 0]]):
        with pytest.raises(ValueError, match="slots"):
            RO.playout_value(recs, 2, SEED, rules="host", move_values=many, slots=bad)
    moves, won = histories(recs, 1)
    with pytest.raises(TypeError, match="slots"):
        MV.move_value_update_host(many, recs, moves, won, 3, 1)
    with pytest.raises(TypeError, match="slots"):
        MV.move_value_update_host(MV.MoveValueTable.empty(), recs, moves, won, 3, 1, slots=slots)
    with pytest.raises(ValueError, match="slots"):
        MV.move_value_update_host(many, recs, moves, won, 3, 1, slots=slots[:2])
    assert not many.counts.any()
    for f in (T.move_value_playouts, T.move_value_update, MV.move_value_update_host, MV.move_value_weights):
        assert inspect.signature(f).parameters["slots"].default is None


# ---- 3. the evaluator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more,single", [(dict(), dict()), (dict(pair_games=3), dict(replies=2)),
                                         (dict(replies=True, games=3), dict(replies=True))])
def test_the_evaluator_with_a_move_value_table_per_game(more, single):
    same = lambda x: x                                                # noqa: E731
    base = dict(seed=4, prior=1.0, rave=True, rules="host")
    runs = []
    for _ in range(2):
        ev = RO.PlayoutEvaluator(None, 4, move_value_games=3, move_value_tau=0.1, **more, **base)
        assert ev.wants_games is True and type(ev.move_values) is MV.MoveValueTables and ev.move_values.count == 3
        assert np.array_equal(ev.move_values.lut, MV.lut_of(0.1))
        runs.append([_bits(ev.finish(ev.submit(r, n, games=g), normalise=same)) for r, n, g in requests()] + [ev.move_values.copy()])
    assert runs[0][:3] == runs[1][:3] and same_tables(runs[0][3], runs[1][3])         # the same bits when run twice
    assert all(runs[0][3].table(i).occupancy() > 50 for i in range(3))
    with pytest.raises(TypeError, match="games"):
        ev.submit(requests()[0][0], 2)
    # a game's table is that game's rows evaluated alone, in their own order, through PlayoutEvaluator(move_values=tau)
    for game in range(3):
        alone = RO.PlayoutEvaluator(None, 4, move_values=0.1, **single, **base)
        for r, n, g in requests():
            rows = np.nonzero(g == game)[0]
            alone.finish(alone.submit(r[rows], 0), normalise=same)
        assert same_tables(alone.move_values, runs[0][3].table(game)), game
        if single:
            assert np.array_equal(alone.replies.array, ev.replies.array[game]), game
    ev.reset_move_values()
    assert not ev.move_values.counts.any() and (ev.move_values.values == 256).all()
    # not the values of the evaluator without the tables
    plain = RO.PlayoutEvaluator(None, 4, **more, **base)
    other = [_bits(plain.finish(plain.submit(r, n, **(dict(games=g) if more else {})), normalise=same)) for r, n, g in requests()]
    assert other[0] == runs[0][0] and other != runs[0][:3]            # fresh tables are neutral: the first request is the plain one


def test_what_the_evaluator_refuses_and_what_stays_what_it_is():
    base = dict(seed=4, prior=1.0, rules="host")
    for kw in (dict(move_values=True), dict(move_values=0.1), dict(replies=True), dict(replies=2)):
        with pytest.raises(TypeError, match="move_value_games"):
            RO.PlayoutEvaluator(None, 4, move_value_games=3, **kw, **base)
    for kw in (dict(replies=True, games=2), dict(pair_games=4)):
        with pytest.raises(ValueError, match="equally many"):
            RO.PlayoutEvaluator(None, 4, move_value_games=3, **kw, **base)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            RO.PlayoutEvaluator(None, 4, move_value_games=bad, **base)
    with pytest.raises(ValueError):
        RO.PlayoutEvaluator(None, 4, move_value_games=2, move_value_tau=0.0, **base)
    for kw in (dict(replies=True, games=3), dict(pair_games=3)):      # the pinned refusals
        with pytest.raises(TypeError, match="games"):
            RO.PlayoutEvaluator(None, 4, move_values=True, **kw, **base)
    params = inspect.signature(RO.PlayoutEvaluator.__init__).parameters
    assert params["move_value_games"].default is None and params["move_value_tau"].default == MV.DEFAULT_TAU
    ev = RO.PlayoutEvaluator(None, 4, **base)
    assert ev.move_values is None and ev.wants_games is False
    with pytest.raises(TypeError, match="move-value"):
        ev.reset_move_values()
    ev = RO.PlayoutEvaluator(None, 4, move_value_games=2, **base)
    assert ev.replies is None and np.array_equal(ev.move_values.lut, MV.lut_of(MV.DEFAULT_TAU))


# ---- 4. self_play ---------------------------------------------------------------------------------------------------------------
def _evaluator(**kw):
    return RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, move_value_games=3, rules="host", **kw)


def _play(ev=None, **kw):
    ev = _evaluator() if ev is None else ev
    local, _ = selfplay.self_play(ev, **dict(KW, rave=4, **kw))
    assert local["native_loop"] is False and local["dedup"] is False
    return {g: (v["moves"], local["visits"][g]) for g, v in local["games"].items()}, ev


@pytest.fixture(scope="module")
def played():
    ev = _evaluator()
    ev.move_values.values[...] = 7                                    # self_play clears the tables first
    ev.move_values.counts[...] = 3
    return _play(ev)


def test_self_play_gives_every_game_its_own_move_value_table(played):
    games, ev = played
    assert sorted(games) == [0, 1, 2] and all(len(m) > 0 and len(v) == len(m) for m, v in games.values())
    assert all(ev.move_values.table(g).occupancy() > 50 for g in range(3))
    for g in range(3):                                                # a game is a pure function of seed_base + gid; its table
        alone, ev1 = _play(gids=[g])                                  # is the one a fresh evaluator learns: the 7s were cleared
        assert alone == {g: games[g]}, g
        assert same_tables(ev1.move_values.table(0), ev.move_values.table(g)) and not ev1.move_values.counts[1:].any()
    for kw in (dict(n_pools=2, threads=3), dict(pool_sizes=[2, 1])):  # against the fixture's one pool on one thread
        assert _play(**kw)[0] == games, kw
    plain, _ = _play(RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, replies=True, games=3, rules="host"))
    both, ev2 = _play(_evaluator(replies=True, games=3))              # beside a reply table per game
    assert plain != games and both != games and both != plain
    assert (ev2.replies.occupancy() > 0).all() and all(ev2.move_values.table(g).occupancy() > 50 for g in range(3))
    with pytest.raises(ValueError, match="move-value tables"):        # two tables, three games
        selfplay.self_play(RO.PlayoutEvaluator(None, 8, prior=1.0, move_value_games=2, rules="host"), **KW)
    with pytest.raises(ValueError, match="native_loop"):
        _play(native_loop=True)
    with pytest.raises(ValueError, match="dedup"):
        _play(dedup=True)


def test_a_one_game_pool_equals_the_single_table_evaluator_driven_by_hand(played):
    games, _ = played
    g = 2
    ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, move_values=MV.DEFAULT_TAU, rules="host")   # DESIGN 30's: one table
    prm = selfplay.search_params(rollouts=16, expand_thresh=2, noise_weight=0.25, sample_plies=2, max_turns=6, prune=1,
                                 record_visits=1, eager_top=2, speculate=0, speculate_rows=8, leaves=1, leaves_visit_only=0)
    pool = selfplay.GamePool([20260 + g], prm, cap=200, threads=1)
    pool.set_task_cap(0)
    pool.set_rave(4)
    while True:
        recs, npol = pool.collect_positions()
        if len(recs) == 0:
            break
        pool.deliver(*ev.finish(ev.submit(recs, npol), normalise=selfplay.normalise_rows))
    moves = pool.moves(0)
    assert (moves, [pool.visits(0, ply) for ply in range(len(moves))]) == games[g]
    pool.close()


# ---- 5. the command line ------------------------------------------------------------------------------------------------------
def test_the_flag_of_selfplay(capsys):
    a = selfplay.parse_args(["--playout-value", "64", "--playout-prior", "1", "--game-rave", "--game-reply-pairs", "--game-move-values"])
    assert a.game_move_values == 0.25 and a.game_reply_pairs is True and a.game_rave == 4.0
    assert selfplay.game_table_keywords(a, 5) == dict(pair_games=5, move_value_games=5, move_value_tau=0.25)
    a = selfplay.parse_args(["--playout-value", "8", "--game-replies", "--game-move-values", "0.1"])
    assert a.game_move_values == 0.1
    assert selfplay.game_table_keywords(a, 2) == dict(replies=True, games=2, move_value_games=2, move_value_tau=0.1)
    a = selfplay.parse_args(["--playout-value", "8", "--game-move-values"])
    assert selfplay.game_table_keywords(a, 3) == dict(move_value_games=3, move_value_tau=0.25)
    RO.PlayoutEvaluator(None, 4, prior=1.0, rules="host", **selfplay.game_table_keywords(a, 3))
    a = selfplay.parse_args(["--playout-value", "8", "--game-replies"])
    assert a.game_move_values == 0.0 and selfplay.game_table_keywords(a, 2) == dict(replies=True, games=2)
    a = selfplay.parse_args([])
    assert a.game_move_values == 0.0 and selfplay.game_table_keywords(a, 2) == {}
    with pytest.raises(SystemExit):
        selfplay.parse_args(["--game-move-values"])
    err = capsys.readouterr().err
    assert "--game-move-values" in err and "--playout-value" in err
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            selfplay.parse_args(["--playout-value", "8", "--game-move-values", bad])
        assert "--game-move-values" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                   # still not selfplay's
        selfplay.parse_args(["--playout-value", "8", "--playout-move-values"])
    capsys.readouterr()
    assert "move_value_games" in selfplay.self_play.__doc__
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "--game-rave --game-reply-pairs --game-move-values" in readme
    assert "game_move_values_bench.py" in open(os.path.join(REPO, "tools", "README.md")).read()
    assert re.search(r"^## 31\.", open(os.path.join(REPO, "DESIGN.md")).read(), flags=re.M)


# ---- 6. header, bindings, build -----------------------------------------------------------------------------------------------
def test_header_bindings_makefile_and_the_kernels_names():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_MAX_MOVE_VALUE_TABLES\s+4096\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_move_value_playouts_tables\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*const\s+uint16_t\s*\*\s*values\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*replies\s*,\s*const\s+uint8_t\s*\*\s*replies2\s*,\s*int\s+tables\s*,"
                     r"\s*const\s+int32_t\s*\*\s*slots\s*,\s*int\s+max_plies\s*,\s*uint8_t\s*\*\s*over\s*,"
                     r"\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,\s*int32_t\s*\*\s*status\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bsize_t\s+bkt_move_value_tables_scratch_bytes\s*\(\s*int\s+records\s*,\s*int\s+tables\s*\)", code)
    assert re.search(r"\bint\s+bkt_move_value_update_tables\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*const\s+int16_t\s*\*\s*moves\s*,"
                     r"\s*int\s+max_plies\s*,\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*int64_t\s*\*\s*counts\s*,\s*uint16_t\s*\*\s*values\s*,\s*const\s+uint16_t\s*\*\s*lut\s*,\s*int\s+k\s*,"
                     r"\s*int\s+limit\s*,\s*int\s+tables\s*,\s*const\s+int32_t\s*\*\s*slots\s*,\s*void\s*\*\s*scratch\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("counts int64 [tables][2][81][2]", "values uint16 [tables][2][81]", "1 <= tables <= BKT_MAX_MOVE_VALUE_TABLES",
                   "slots int32 [batch] for the playouts, [records] for the update",
                   "A slot outside 0..tables-1 is compared before it indexes anything",
                   "such a row plays as if every value were 256, and such a record updates nothing",
                   "replies is NULL or uint8 [tables][162]", "replies2 is NULL or uint8 [tables][2][82][81], 4-byte aligned",
                   "at most one of replies and replies2 may be given",
                   "The same slots and the same tables name the reply table and the move-value table of a row",
                   "it is bkt_move_value_playouts byte for byte", "it is bkt_move_value_update byte for byte",
                   "A table that is named gets every entry of values written", "A table that no record names keeps every byte",
                   "A record with a slot outside the range updates nothing", "A refused call launches nothing and writes nothing"):
        assert " ".join(phrase.replace("*", " ").split()) in flat, phrase
    P, I, U64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t
    assert T.SYMBOLS["bkt_move_value_playouts_tables"] == (I, [P, I, U64, P, P, P, P, P, P, I, P, I, P, P, P, P, P])
    assert T.SYMBOLS["bkt_move_value_tables_scratch_bytes"] == (Z, [I, I])
    assert T.SYMBOLS["bkt_move_value_update_tables"] == (I, [P, P, I, P, I, I, P, P, P, I, I, I, P, P, P])
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        lib.bkt_move_value_tables_scratch_bytes.restype, lib.bkt_move_value_tables_scratch_bytes.argtypes = Z, [I, I]
        assert lib.bkt_abi_version() == 4 and lib.bkt_move_value_playouts_tables and lib.bkt_move_value_update_tables
        assert [lib.bkt_move_value_tables_scratch_bytes(n, t) for n, t in ((-1, 1), (0, 1), (1, 1), (3, 4096), (3, 0), (3, 4097), (1024, 7))] \
            == [0, 0, 1296, 3888, 0, 0, 1024 * 1296]
    # the Makefile: the draw's file a dependency only, the update's a source in front of -shared beside the single table's
    make = open(os.path.join(CSRC, "Makefile")).read()
    rule, line = re.search(r"^\$\(TRAIN_OUT\):(.*)\n\t(.*)$", make, flags=re.M).groups()
    assert "bk_playout_mast_tables.hip" in rule.split() and "bk_playout_mast_tables.hip" not in line.split()
    front = line.split("-shared")[0].split()
    assert "bk_playout_mast_tables_update.hip" in rule.split() and "bk_playout_mast_tables_update.hip" in front
    assert front.index("bk_playout_mast_tables_update.hip") == front.index("bk_playout_mast_update.hip") + 1
    # included as text at the very end of bk_playout_mast.hip, behind its closing brace and its entry point
    host = open(os.path.join(CSRC, "bk_playout_mast.hip")).read()
    assert re.findall(r'^#include "([^"]+)"', host, flags=re.M) == ["bk_playout_mast_tables.hip"]
    assert host.rstrip().splitlines()[-1].startswith('#include "bk_playout_mast_tables.hip"')
    assert host.index("bkt_move_value_playouts(") < host.index('#include "bk_playout_mast_tables.hip"')
    draw, update = (open(os.path.join(CSRC, name)).read() for name in ("bk_playout_mast_tables.hip", "bk_playout_mast_tables_update.hip"))
    for own in (draw, update):
        assert "float" not in own and "double" not in own and not re.search(r"\batomic\w*\s*\(", own)
    assert "__syncthreads" not in draw and "#include" not in draw
    for inst in ("WeightedDraw<GameMoveValueWeight>{", "ReplyDraw<WeightedDraw<GameMoveValueWeight>, PPW>",
                 "GamePairsDraw<WeightedDraw<GameMoveValueWeight>>"):
        assert inst in draw, inst
    new = kernels_of("bk_playout_mast_tables.hip")
    assert len(new) == 3 and len(set(new)) == 3 and all(k.startswith("gamevalues_") for k in new), new
    both = new + kernels_of("bk_playout_mast_tables_update.hip")
    assert len(both) == 5 and len(set(both)) == 5 and all(k.startswith("gamevalues_") for k in both), both
    existing = OLD_KERNELS + ("gamepairs_", "movevalue_", "balance_sums_kernel", "amaf_counts", "reply_tables_")
    assert not [(k, old) for k in both for old in existing if old in k]
    assert len(kernels_of("bk_playout_mast.hip")) == 3 and len(kernels_of("bk_playout_mast_update.hip")) == 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_new_kernels_keep_the_resource_conditions_beside_their_siblings(tmp_path):
    """Zero spills and zero scratch in every kernel of the playout translation unit; the three new playout kernels at an
    occupancy of at least the tactical kernel's, itself at least 4, within 128 VGPRs, and with at most the three staged
    tables' 972 bytes and 16 of alignment more LDS than the kernel each is the per-game sibling of; the two update kernels
    without spills or scratch."""
    err, blocks, fields = resources("bk_playout_pat.hip", tmp_path)
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", err)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)
    assert len(spills) == 2 * len(blocks) and len(scratch) == len(blocks)
    assert all(int(n) == 0 for _, n in spills) and all(int(n) == 0 for n in scratch), (spills, scratch)
    tactical = fields("tactical_playouts_kernel")
    for new, sibling in (("gamevalues_draw_kernel", "tactical_playouts_kernel"), ("gamevalues_single_kernel", "reply_tables_playouts_kernel"),
                         ("gamevalues_pairs_kernel", "gamepairs_weighted_kernel")):
        f, g = fields(new), fields(sibling)
        print(new, f, sibling, g)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (new, f)
        assert f["occupancy"] >= tactical["occupancy"] >= 4 and f["vgprs"] <= 128, (new, f, tactical)
        assert f["lds"] <= g["lds"] + 972 + 16, (new, f, g)
    _, blocks, fields = resources("bk_playout_mast_tables_update.hip", tmp_path)
    assert len(blocks) == 2
    for name in ("gamevalues_counts_kernel", "gamevalues_apply_kernel"):
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0 and f["occupancy"] >= 4, (name, f)

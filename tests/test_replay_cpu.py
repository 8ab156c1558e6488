"""CPU: the one lock-step replay of recorded games (bokego_amd/replay.py) -- what the four fitting modules compute
through it on the host rules against pins taken before they shared it, the host walker itself against go.Game, and the one
weight-table class behind PatternTable and TacticTable."""
import hashlib
import json
import os

import numpy as np
import pytest

from bokego_amd import balance as B
from bokego_amd import go
from bokego_amd import lockstep as L
from bokego_amd import mmfit as M
from bokego_amd import patterns as PT
from bokego_amd import replay as R
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from conftest import GOLDEN
from test_rollout_cpu import BOARD, records

PINS = os.path.join(GOLDEN, "replay_pins.json")
NONE = RO.MOVE_NONE
LENGTHS = (30, 12, 0, 45, 20, 33, 8)               # plies kept of each game; at batch=3: (30, 12, 0), (45, 20, 33), (8,)
EVAL_PLIES = (0, 5, 9, 31, 40)
LABEL_PLIES = (0, 8, 20, 44)


def game_set():
    """(start uint8 [7,192], moves int16 [7,45]): seven uniform host-rule games from the empty board, cut by hand to
    LENGTHS -- game 2 is all MOVE_NONE, and game 1 ends in a pass that is followed by MOVE_NONE."""
    start = L.initial_positions(len(LENGTHS))
    moves = RO.random_playouts(start, 29, max_plies=max(LENGTHS), rules="host").moves.copy()
    assert moves.shape == (len(LENGTHS), max(LENGTHS)) and (moves >= 0).all()          # no game ends this early
    for g, n in enumerate(LENGTHS):
        moves[g, n:] = NONE
    moves[1, LENGTHS[1] - 1] = go.PASS
    return start, moves


def tables():
    rng = np.random.default_rng(31)
    return (PT.PatternTable(rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16)),
            TC.TacticTable(rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16)))


def digest(a):
    a = np.ascontiguousarray(a)
    return f"{a.dtype} {list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}"


def compute_pins():
    """What the fitting modules make of game_set() on the host rules, through public names only: the digest of every
    array (integers, and the float64 mass and targets, by their bytes), the mass itself as the hex of its bytes (the device's
    is compared with it), and evaluate's dicts as they are."""
    start, moves = game_set()
    table, tac = tables()
    out = {}
    out["patterns.counts"] = [digest(a) for a in PT.counts(start, moves, rules="host")]
    for name, pat in (("tactics.counts", None), ("tactics.counts(patterns)", table)):
        mass, played = TC.counts(start, moves, pat, rules="host")
        out[name] = [digest(mass), digest(played), mass.tobytes().hex()]
    out["mmfit.pack"] = [digest(a) for a in M.pack(start, moves, rules="host")]
    out["mmfit.evaluate"] = M.evaluate(start, moves, table, tac, rules="host")
    out["mmfit.evaluate(plies)"] = M.evaluate(start, moves, table, tac, rules="host", plies=EVAL_PLIES)
    out["balance.labelled_positions"] = [digest(a) for a in B.labelled_positions(start, moves, plies=LABEL_PLIES)]
    return out


# ---- the pins ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def computed():
    return compute_pins()


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


def test_the_game_set_has_the_edges_the_pins_are_for():
    start, moves = game_set()
    assert [(row > NONE).sum() for row in moves] == list(LENGTHS) and (moves[2] == NONE).all()
    assert moves[1, LENGTHS[1] - 1] == go.PASS and moves[1, LENGTHS[1]] == NONE


@pytest.mark.parametrize("name", ["patterns.counts", "tactics.counts", "tactics.counts(patterns)", "mmfit.pack",
                                  "balance.labelled_positions"])
def test_arrays_keep_their_bits(computed, pins, name):
    assert computed[name] == pins[name]


@pytest.mark.parametrize("name", ["mmfit.evaluate", "mmfit.evaluate(plies)"])
def test_evaluate_keeps_its_counts_and_its_likelihood(computed, pins, name):
    got, want = computed[name], pins[name]
    assert sorted(got) == sorted(want) == ["mean_ll", "moves", "top1", "top5"] and want["moves"] > 0
    assert all(got[f] == want[f] for f in ("moves", "top1", "top5"))
    assert abs(got["mean_ll"] - want["mean_ll"]) <= 1e-12 * abs(want["mean_ll"])       # np.log: the last place may differ
    assert pins["mmfit.evaluate(plies)"]["moves"] < pins["mmfit.evaluate"]["moves"]


# ---- the host walker --------------------------------------------------------------------------------------------------------------
def by_game_set_replay():
    """{(game, ply): the record before that ply}, by go.Game alone."""
    start, moves = game_set()
    out = {}
    for g, row in enumerate(moves.tolist()):
        game = go.Game()
        for k, mv in enumerate(row):
            if mv > NONE:
                out[g, k] = records([game])[0]
                game.play_pass() if mv == go.PASS else game.play_move(mv)
                game.get_liberties()                                  # the record carries its liberty cache, as the device's does
    return out


def walk(batch, playable=True):
    """{(game, ply): (record, move, playable set)} of a walk, with the checks every walk must pass on the way."""
    start, moves = game_set()
    before, out, last = start.copy(), {}, (0, -1)
    for k, first, live, recs, mv, ok in R.replay_host(start, moves, batch, playable=playable):
        assert (first, k) > last and len(live) and (np.diff(live) > 0).all() and len(recs) <= (batch or len(start))
        last = (first, k)
        assert np.array_equal(mv, moves[first + live, k]) and (ok is None) == (not playable)
        for i, g in enumerate((first + live).tolist()):
            out[g, k] = (recs[live[i]].copy(), int(mv[i]), None if ok is None else ok[i].copy())
    assert np.array_equal(start, before)                                               # the walker plays on a copy
    return out


def test_the_host_walker_against_go_game():
    want, got = by_game_set_replay(), walk(3)
    assert sorted(got) == sorted(want) and len(want) == sum(LENGTHS)
    # batch 0 holds no live game from ply 30 on, batch 2 none from ply 8 on, while batch 1 runs to ply 44
    assert (3, 44) in got and (0, 29) in got and (0, 30) not in got and (6, 7) in got
    for key, rec in want.items():
        assert np.array_equal(got[key][0], rec), key
        assert np.array_equal(got[key][2], RO.playable_host(rec[None])[0]), key


@pytest.mark.parametrize("batch", [3, 1, 7, 100])
def test_batches_walk_the_same_games(batch):
    whole, parts = walk(None), walk(batch, playable=batch == 3)
    assert sorted(whole) == sorted(parts)
    for key in whole:
        assert np.array_equal(whole[key][0], parts[key][0]) and whole[key][1] == parts[key][1], key
        assert parts[key][2] is None or np.array_equal(whole[key][2], parts[key][2])


def test_what_the_walker_refuses():
    occupied = np.array([[1]], np.int16)                                              # test_patterns_cpu's case: a stone lies there
    with pytest.raises(RuntimeError, match=r"^game 0: the recorded move 1 is illegal$"):
        list(R.replay_host(records([go.Game(BOARD)]), occupied))
    start = records([go.Game(), go.Game(), go.Game(), go.Game(BOARD)])
    late = np.array([[40, 41]] * 3 + [[38, 38]], np.int16)                            # game 3, in the second batch of 3
    with pytest.raises(RuntimeError, match=r"^game 3: the recorded move 38 is illegal$"):
        list(R.replay_host(start, late, 3))
    for fn in (PT.counts, TC.counts, M.pack, M.evaluate):
        with pytest.raises(RuntimeError, match="game 0: the recorded move 1 is illegal"):
            fn(records([go.Game(BOARD)]), occupied, rules="host")
    with pytest.raises(RuntimeError, match="game 0: the recorded move 1 is illegal"):
        B.labelled_positions(records([go.Game(BOARD)]), occupied, plies=(0,))
    for bad in (np.array([40], np.int16), np.zeros((2, 3), np.int16)):                 # 1-D moves; moves of another game count
        with pytest.raises(ValueError, match=r"records uint8 \[G,192\] and their moves \[G,L\]"):
            R.check_games(records([go.Game()]), bad)
        for fn in (PT.counts, TC.counts, M.pack, M.evaluate, B.labelled_positions):
            with pytest.raises(ValueError):
                fn(records([go.Game()]), bad)


def test_the_small_helpers():
    import torch
    mv = np.array([-1, 0, 5, 80, 7], np.int32)
    ok = np.zeros((5, 81), bool)
    ok[0, 0] = ok[2, 5] = ok[3, 79] = ok[4, 7] = True
    codes = np.arange(5 * 81).reshape(5, 81)
    at, good = R.counted(mv, ok)
    assert good.tolist() == [False, False, True, False, True] and R.at_move(codes, at).tolist() == [0, 81, 167, 323, 331]
    at_t, good_t = R.counted(torch.from_numpy(mv), torch.from_numpy(ok))
    assert good_t.tolist() == good.tolist() and R.at_move(torch.from_numpy(codes), at_t).tolist() == [0, 81, 167, 323, 331]
    # the rank: heavier candidates, and equally heavy ones at a lower point; only candidates count
    w = np.array([[5, 9, 5, 5, 0, 9] + [0] * 75], np.int64)
    for move, want in ((1, 0), (5, 1), (0, 2), (2, 3), (3, 4)):
        assert R.move_rank(w, w[:, move], np.array([move]), w > 0).tolist() == [want]


# ---- the one table class ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls, noun, entries", [(PT.PatternTable, "pattern", PT.ENTRIES), (TC.TacticTable, "tactics", TC.ENTRIES)])
def test_both_tables_are_one_class(tmp_path, cls, noun, entries):
    assert issubclass(cls, PT.WeightTable) and cls.ENTRIES == entries
    table = cls(np.random.default_rng(4).integers(0, 65536, entries).astype(np.uint16))
    for bad in (np.zeros(entries, np.int16), np.zeros(entries, np.float32), np.zeros(entries + 1, np.uint16),
                np.zeros((2, entries // 2), np.uint16)):
        with pytest.raises(ValueError) as e:
            cls(bad)
        assert str(e.value) == f"a {noun} table is uint16 [{entries}], got {bad.dtype} {bad.shape}"
    path = str(tmp_path / "table.npy")
    table.save(path)
    assert np.array_equal(cls.load(path).array, table.array) and np.array_equal(np.load(path), table.array)
    assert np.array_equal(table.entries(np.array([[0, entries - 1]])), table.array[[0, entries - 1]][None])
    assert cls.coerce(None) is None and cls.coerce(table) is table
    assert np.array_equal(cls.coerce(table.array).array, table.array) and np.array_equal(cls.coerce(path).array, table.array)
    assert PT.as_table(None) is None and TC.as_tactics(None) is None
    assert isinstance(PT.as_table(PT.PatternTable.constant(3).array), PT.PatternTable)
    assert isinstance(TC.as_tactics(TC.TacticTable.neutral().array), TC.TacticTable)


def test_the_names_that_moved_are_still_where_they_were():
    assert RO.playable_host is L.playable_host and "playable_host" in RO.__all__
    assert PT.record_games is R.record_games

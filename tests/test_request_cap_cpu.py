"""One layer above the kernels: the native tree's requests against the `cap` of a collect (include/bokego_tree.h).

A game whose request does not fit under `cap` keeps it for the next collect; a request that can NEVER fit is skipped for ever,
collect returns 0 rows, and every driver reads 0 rows as "all games are over".  These tests run the multi-leaf mode (leaves > 1)
at caps that bind, and check what a driver that returned left behind: every collect within `cap`, every game done, every ply's
record complete, the games a pure function of their seeds; an oversize request is an error code, not an end; self_play never
reduces over an unfinished game; bk_pool_create and bk_pool_restore accept the same parameters; and the virtual loss is only used
where its scale is the backup's (value_weight == 1).

`python tests/test_request_cap_cpu.py` rewrites tests/golden/multi_leaf_games.json (recorded before search_leaves() learnt about
row_cap: a cap that does not bind must change nothing)."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN            # (first: it puts the repository on the path when this file runs as the golden's writer)

from bokego_amd import go, selfplay
from test_native_mcts_cpu import FakeNets

F = FakeNets()
EV = selfplay.CallableEvaluator(F.policy, F.value)          # planes (GamePool.collect)
REC = selfplay.RecordEvaluator(F.policy, F.value)           # position records (GamePool.collect_positions)
GOLDEN_GAMES = os.path.join(GOLDEN, "multi_leaf_games.json")
ERR_ARG, ERR_OVERSIZE = -1, -82                             # BK_POOL_ERR_ARG, BK_POOL_ERR_OVERSIZE (include/bokego_tree.h)
CAPS = (82, 83, 128, 164, 4096)


def _ended(moves, max_turns):
    """A pool's game ends when the turn passes max_turns (max_turns + 1 moves) or on passes."""
    return len(moves) == max_turns + 1 or (len(moves) >= 2 and moves[-1] == go.PASS and moves[-2] == go.PASS)


def _drive(pool, mode, cap, limit=200_000):
    """collect / deliver by hand until collect returns 0 rows; every batch within cap.  mode: 'feats' = bk_pool_collect,
    'pos' = bk_pool_collect_pos, 'dedup' = the same with in-batch de-duplication."""
    ev = EV if mode == "feats" else REC
    pool.set_dedup(mode == "dedup")
    biggest = 0
    for _ in range(limit):
        rows, npol = pool.collect() if mode == "feats" else pool.collect_positions()
        assert len(rows) <= cap and 0 <= npol <= len(rows)
        if len(rows) == 0:
            return biggest
        biggest = max(biggest, len(rows))
        pool.deliver(*ev.finish(ev.submit(rows, npol), normalise=selfplay.normalise_rows))
    raise AssertionError("the pool never came to an end")


def _check_finished(pool, n_games, rollouts, max_turns):
    for g in range(n_games):
        info, moves = pool.info(g), pool.moves(g)
        assert info["done"] == 1, (g, info)                      # collect returned 0: every game is over
        assert _ended(moves, max_turns), (g, moves)
        for ply in range(len(moves)):                            # every ply's record holds that ply's rollouts (+ the kept subtree's)
            assert sum(pool.visits(g, ply).values()) >= rollouts - 1, (g, ply)


# ---- no request outgrows a collect, and every game ends --------------------------------------------------------------------------
def _grid():
    """(id, search parameters, seeds, cap, mode): leaves x eager_top (0 = every child) with caps, the kind of virtual loss and the
    driver cycling through; every cap again for the two largest leaves with every child evaluated; and by name the two
    configurations that stalled before search_leaves() asked room_for_rows."""
    modes = ("feats", "pos", "dedup")
    shapes = ((2, 60, 8, 11), (3, 120, 4, 12), (4, 400, 2, 10))          # games, rollouts, expand_thresh, max_turns
    out, seen, k = [], set(), 0

    def add(leaves, top, vo, cap, name=None, shape=None, mode=None, **extra):
        nonlocal k
        if name is None and (leaves, top, vo, cap) in seen:
            return
        seen.add((leaves, top, vo, cap))
        n, r, t, m = shape or shapes[k % 3]
        kw = dict(rollouts=r, expand_thresh=t, max_turns=m, record_visits=1, leaves=leaves, eager_top=top, leaves_visit_only=vo,
                  noise_weight=0.25, sample_plies=3, **extra)
        md = mode or modes[k % 3]
        out.append(pytest.param(kw, [77 + i for i in range(n)], cap, md, id=name or f"leaves{leaves}-top{top}-vo{vo}-cap{cap}-{md}"))
        k += 1

    for li, leaves in enumerate((1, 2, 4, 16, 64)):
        for ei, top in enumerate((0, 2, 4)):
            add(leaves, top, (li + ei) % 2, CAPS[(li + 2 * ei) % 5])
    for leaves in (16, 64):
        for ci, cap in enumerate(CAPS):
            add(leaves, 0, ci % 2, cap)
            add(leaves, 4, 1 - ci % 2, cap)
    for md in modes:
        # GamePool([77, 78], leaves=16, every child, cap=128): game 1 stopped at move 8 with done == 0
        add(16, 0, 0, 128, name=f"stalled-pool-leaves16-cap128-{md}", shape=(2, 60, 8, 11), mode=md)
        # self_play(n_games=4, rollouts=400, expand_thresh=2, max_turns=10, eager_top=0, cap=128, leaves=16 / 4): 0 moves, 4 "white wins"
        add(16, 0, 0, 128, name=f"stalled-selfplay-leaves16-cap128-{md}", shape=(4, 400, 2, 10), mode=md, prune=1)
        add(4, 0, 0, 128, name=f"stalled-selfplay-leaves4-cap128-{md}", shape=(4, 400, 2, 10), mode=md, prune=1)
    return out


@pytest.mark.parametrize("kw,seeds,cap,mode", _grid())
def test_no_request_outgrows_a_collect_and_every_game_ends(kw, seeds, cap, mode):
    pool = selfplay.GamePool(seeds, selfplay.search_params(**kw), cap=cap, threads=1 + len(seeds) % 2)
    biggest = _drive(pool, mode, cap)
    _check_finished(pool, len(seeds), kw["rollouts"], kw["max_turns"])
    assert 0 < biggest <= cap
    pool.close()


def test_run_pools_leaves_every_game_done_at_a_binding_cap():
    """The first configuration of the report, through the Python driver: run_pools returned normally with game 1 at move 8."""
    prm = selfplay.search_params(rollouts=60, expand_thresh=8, noise_weight=0.25, sample_plies=3, max_turns=11, record_visits=1, leaves=16)
    pool = selfplay.GamePool([77, 78], prm, cap=128)
    selfplay.run_pools([pool], EV)
    _check_finished(pool, 2, 60, 11)
    pool.close()


# ---- games stay a pure function at a binding cap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("visit_only,cap", [(0, 128), (1, 300), (0, 300)])
def test_games_are_a_pure_function_of_their_seeds_at_a_binding_cap(visit_only, cap):
    """test_multi_leaf_games_are_a_pure_function_of_their_seeds (tests/test_native_mcts_cpu.py) at leaves=16, every child evaluated,
    and a cap that binds: where a step stops gathering depends on the game's own state and the cap, never on what else is in the
    batch.  cap=128 (the configuration that stalled) holds one expansion's 82 rows and not the 83 another rollout may add: the
    step sends after its first expansion.  cap=300 holds three: the mode is on, the cap binds, and the games are neither the
    one-leaf search's nor those of a cap that does not bind -- the cap is one of the things a multi-leaf game is a function of."""
    kw = dict(n_games=6, rollouts=80, expand_thresh=4, noise_weight=0.25, sample_plies=3, max_turns=10, cap=cap, eager_top=0,
              record_visits=1, leaves=16, leaves_visit_only=visit_only)

    def run(**extra):
        return selfplay.self_play(selfplay.RecordEvaluator(F.policy, F.value), **{**kw, **extra})

    base, tot = run(n_pools=1, threads=1, native_loop=True)
    assert sorted(base["games"]) == list(range(6)) and all(_ended(g["moves"], 10) for g in base["games"].values())
    assert tot["games"] == 6 and tot["plies"] == sum(len(g["moves"]) for g in base["games"].values())
    assert all(sum(ply.values()) >= 80 - 1 for plies in base["visits"].values() for ply in plies)
    for extra in (dict(n_pools=1, threads=1, native_loop=False), dict(n_pools=2, threads=3, native_loop=True),
                  dict(n_pools=3, threads=2, native_loop=False), dict(n_pools=2, threads=2, dedup=True, task_cap=30),
                  dict(n_pools=3, threads=1, dedup=True, task_cap=30, native_loop=False)):
        local, total = run(**extra)
        assert local["games"] == base["games"] and local["visits"] == base["visits"], extra
        assert np.array_equal(total["root_visit_hist"], tot["root_visit_hist"]) and total["sum_root_value"] == tot["sum_root_value"]
    halves = [run(rank=r, world=2, n_pools=2, threads=2) for r in (0, 1)]
    assert {**halves[0][0]["games"], **halves[1][0]["games"]} == base["games"]
    assert {**halves[0][0]["visits"], **halves[1][0]["visits"]} == base["visits"]
    if cap == 300:
        one, _ = run(n_pools=1, threads=1, leaves=1)
        roomy, _ = run(n_pools=1, threads=1, cap=4096)
        assert one["games"] != base["games"] and roomy["games"] != base["games"] and roomy["steps"] < base["steps"] < one["steps"]


# ---- a cap that does not bind changes nothing ------------------------------------------------------------------------------------
class ExactEvaluator(selfplay.RecordEvaluator):
    """Networks whose outputs are the same bits on every host: integer weights on 0/1 planes (every partial sum an exact integer),
    priors 2^k, values d / 64 clipped -- no BLAS, exp or tanh whose rounding could differ between the machine that recorded
    tests/golden/multi_leaf_games.json and the one that checks it.  The row sums are bk_normalise_rows's (C, left to right)."""

    def __init__(self):
        super().__init__(None, None)
        rng = np.random.default_rng(11)
        self.Wp = rng.integers(-6, 7, (2187, 81)).astype(np.int64)
        self.wv = rng.integers(-3, 4, 2187).astype(np.int64)

    def finish(self, handle, normalise=selfplay.normalise_rows):
        feats, npol = handle
        self.positions += len(feats)
        self.batches += 1
        x = feats.reshape(len(feats), -1).astype(np.int64)
        lg = x[:npol] @ self.Wp
        k = np.maximum((lg - lg.max(axis=1, keepdims=True)) // 8, -30) if npol else np.zeros((0, 81), np.int64)
        probs = normalise(np.ldexp(np.float32(1.0), k.astype(np.int32)).astype(np.float32)) if npol else np.zeros((0, 81), np.float32)
        values = np.clip((x @ self.wv).astype(np.float64) / 64.0, -1.0, 1.0).astype(np.float32)
        return probs, values


GOLDEN_KW = dict(n_games=10, rollouts=120, expand_thresh=12, noise_weight=0.25, sample_plies=3, max_turns=10, eager_top=4, record_visits=1,
                 n_pools=1, threads=1)


def _golden_run(leaves, cap, **extra):
    local, _ = selfplay.self_play(ExactEvaluator(), leaves=leaves, cap=cap, **{**GOLDEN_KW, **extra})
    return {"games": {str(g): {"moves": v["moves"], "score": float(v["score"])} for g, v in local["games"].items()},
            "visits": {str(g): [{str(m): n for m, n in ply.items()} for ply in plies] for g, plies in local["visits"].items()}}


@pytest.mark.parametrize("leaves", [4, 8])
def test_a_cap_that_does_not_bind_changes_nothing(leaves):
    """leaves 4 and 8 with four children per expansion: a request is at most leaves x 8 rows, far below 4096.  The ten games and
    their visit records are those recorded before the tree knew about row_cap in search_leaves() -- at cap=4096, at cap=100000, and
    for other pools, threads and the step loop in Python."""
    want = json.load(open(GOLDEN_GAMES))[f"leaves{leaves}"]
    assert len(want["games"]) == 10 and all(_ended(g["moves"], 10) for g in want["games"].values())
    assert _golden_run(leaves, 4096) == want
    assert _golden_run(leaves, 100000, n_pools=2, threads=2) == want
    assert _golden_run(leaves, 4096, n_pools=3, native_loop=False) == want


def test_one_leaf_games_are_the_same_for_every_cap():
    """leaves = 1: a request is at most 82 rows, every cap of the grid can carry it, and the search is the same search."""
    kw = dict(n_games=4, rollouts=60, expand_thresh=4, noise_weight=0.25, sample_plies=3, max_turns=10, eager_top=0, record_visits=1, n_pools=2)
    runs = [selfplay.self_play(selfplay.RecordEvaluator(F.policy, F.value), cap=cap, **kw)[0] for cap in CAPS]
    assert all(_ended(g["moves"], 10) for g in runs[0]["games"].values())
    for cap, r in zip(CAPS, runs):
        assert r["games"] == runs[0]["games"] and r["visits"] == runs[0]["visits"], cap


# ---- an oversize request is an error, not an end ---------------------------------------------------------------------------------
def _raw_collect(pool, cap, pos, buf):
    npol = ctypes.c_int(-7)
    fn = pool._lib.bk_pool_collect_pos if pos else pool._lib.bk_pool_collect
    return fn(pool._h, buf.ctypes.data, int(cap), ctypes.byref(npol)), npol.value


def test_an_oversize_request_is_an_error_not_an_end():
    """The one construction left in which a lone request exceeds `cap`: it was made under a larger cap and is still waiting (the
    batch's task limit left its game out) when a collect with a smaller cap comes.  That collect returns BK_POOL_ERR_OVERSIZE and
    changes nothing -- the next collect with the large cap carries on to the same games -- and so do bk_pools_run, GamePool and
    run_pools_native; a cap below 82 is an argument error."""
    prm = selfplay.search_params(rollouts=60, expand_thresh=4, noise_weight=0.25, sample_plies=3, max_turns=8, record_visits=1, leaves=16)
    lib = selfplay.treelib()
    big = 4096
    twin, pool = (selfplay.GamePool([77, 78], prm, cap=big, threads=1) for _ in range(2))
    buf = np.empty((big, 27 * 81), np.uint8)                      # room for `big` rows of either flavour

    def step(p):
        recs, npol = p.collect_positions()
        out = recs.copy(), npol
        if len(recs):
            p.deliver(*REC.finish(REC.submit(recs, npol), normalise=selfplay.normalise_rows))
        return out

    for p in (twin, pool):
        p.set_task_cap(1)                                         # one game per batch: the other keeps its request and goes first next time
    held = None
    step(twin)
    for _ in range(400):                                          # the twin is one step ahead: its batch is the request `pool` is holding
        step(pool)
        recs, npol = step(twin)
        if len(recs) > 82:
            held = recs, npol
            break
    assert held is not None, "no waiting request ever exceeded 82 rows"
    before = [(pool.moves(g), pool.info(g)) for g in range(2)]
    for pos in (False, True):
        assert _raw_collect(pool, 82, pos, buf)[0] == ERR_OVERSIZE
        assert _raw_collect(pool, 81, pos, buf)[0] == ERR_ARG and _raw_collect(pool, 0, pos, buf)[0] == ERR_ARG
    pool.set_dedup(True)
    assert _raw_collect(pool, 82, True, buf)[0] == ERR_OVERSIZE and _raw_collect(pool, 81, True, buf)[0] == ERR_ARG
    pool.set_dedup(False)
    # the step loop in C passes the code on (and has no request out to wait for)
    handles = (ctypes.c_void_p * 1)(pool._h)
    ev = selfplay.callback_evaluator(REC)
    info = selfplay.RunInfo()
    assert lib.bk_pools_run(handles, 1, ctypes.byref(ev), 82, ctypes.byref(info)) == ERR_OVERSIZE and info.steps == 0
    # ... and still waits for the requests that are out: another pool's batch was submitted before this pool's collect failed
    book = {"out": set(), "waited": []}

    def submit(_ctx, recs, B, n_policy, probs, values):
        book["out"].add(len(book["out"]) + 1)
        return len(book["out"])

    def wait(_ctx, ticket):
        book["waited"].append(int(ticket))
        return 0

    other = selfplay.GamePool([5], prm, cap=big, threads=1)
    counting = selfplay.EvaluatorStruct(None, selfplay._SUBMIT_FN(submit), selfplay._WAIT_FN(wait))
    both = (ctypes.c_void_p * 2)(other._h, pool._h)
    assert lib.bk_pools_run(both, 2, ctypes.byref(counting), 82, ctypes.byref(info)) == ERR_OVERSIZE
    assert book["out"] == {1} and book["waited"] == [1] and info.steps == 1
    other.close()
    pool.cap = 82
    for call in (pool.collect, pool.collect_positions, lambda: selfplay.run_pools_native([pool], REC), lambda: selfplay.run_pools([pool], REC),
                 lambda: selfplay.run_pools([pool], EV)):
        with pytest.raises(RuntimeError, match="exceeds"):
            call()
    pool.cap, pool._feats = big, None                             # (the planes' buffer was sized for 82 rows)
    assert [(pool.moves(g), pool.info(g)) for g in range(2)] == before
    # unchanged: the next collect with the large cap is the twin's batch, row for row, and both play on to the same games
    recs, npol = pool.collect_positions()
    assert npol == held[1] and np.array_equal(recs, held[0])
    pool.deliver(*REC.finish(REC.submit(recs, npol), normalise=selfplay.normalise_rows))
    selfplay.run_pools([pool], REC)
    selfplay.run_pools([twin], REC)
    _check_finished(pool, 2, 60, 8)
    for g in range(2):
        assert pool.moves(g) == twin.moves(g) and pool.info(g) == twin.info(g)
        assert [pool.visits(g, k) for k in range(len(pool.moves(g)))] == [twin.visits(g, k) for k in range(len(twin.moves(g)))]
    # a fresh pool: a cap below 82 is refused before anything is advanced
    fresh = selfplay.GamePool([5], prm, cap=big, threads=1)
    for pos in (False, True):
        assert _raw_collect(fresh, 81, pos, buf)[0] == ERR_ARG
    assert fresh.info(0)["n_nodes"] == 0 and _raw_collect(fresh, 82, True, buf)[0] == 82      # the root's policy row and its 81 children
    for p in (pool, twin, fresh):
        p.close()


# ---- self_play never reduces over an unfinished game -----------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["collect_positions", "collect"])
def test_self_play_refuses_to_reduce_over_unfinished_games(monkeypatch, flavour):
    """A driver that comes back early -- here a collect that reports 0 rows after a few steps -- must not have its games counted:
    four empty games used to come out as `games: 4, white_wins: 4, plies: 0`."""
    real = getattr(selfplay.GamePool, flavour)
    calls = {"n": 0}

    def early(self):
        calls["n"] += 1
        if calls["n"] > 6:
            return (np.empty((0, 192), np.uint8) if flavour == "collect_positions" else np.empty((0, 27, 9, 9), np.uint8)), 0
        return real(self)

    monkeypatch.setattr(selfplay.GamePool, flavour, early)
    ev = selfplay.RecordEvaluator(F.policy, F.value) if flavour == "collect_positions" else selfplay.CallableEvaluator(F.policy, F.value)
    kw = dict(n_games=4, rollouts=30, expand_thresh=4, max_turns=6, cap=256, eager_top=4, n_pools=2, threads=1, native_loop=False, gids=[11, 12, 13, 14])
    with pytest.raises(RuntimeError, match=r"unfinished.*\b11\b.*\b14\b"):
        selfplay.self_play(ev, **kw)
    monkeypatch.undo()
    local, total = selfplay.self_play(ev, **kw)                      # the same call, undisturbed
    assert total["games"] == 4 and total["plies"] == 4 * 7 and all(len(g["moves"]) == 7 for g in local["games"].values())


# ---- create and restore agree ----------------------------------------------------------------------------------------------------
def _param_grid():
    base = dict(leaves=1, eager=1, use_value=1, simulate=0, branch_num=0, value_weight=1.0, speculate=0)
    pts = []

    def add(**kw):
        p = dict(base, **kw)
        if p not in pts:
            pts.append(p)

    for leaves in (0, 1, 64, 65, 100):
        for eager in (0, 1, 2):
            add(leaves=leaves, eager=eager)
        for w in (0.0, 0.5, 1.0):
            add(leaves=leaves, value_weight=w)
        for bn in (0, 5, 81):
            add(leaves=leaves, branch_num=bn)
        add(leaves=leaves, speculate=3)
        add(leaves=leaves, speculate=3, eager=2, branch_num=81)
        for uv, sim in ((0, 0), (0, 1), (1, 1)):
            add(leaves=leaves, use_value=uv, simulate=sim, value_weight=0.5 if uv and sim else (1.0 if uv else 0.0))
    for eager, bn, w, (uv, sim) in itertools.product((0, 2), (5, 81), (0.0, 0.5), ((0, 0), (0, 1), (1, 1), (1, 0))):
        add(leaves=4, eager=eager, branch_num=bn, value_weight=w, use_value=uv, simulate=sim, speculate=3)
    return pts


def _play_on_from_snapshots(kw, n_snapshots):
    """-> None if bk_pool_create refuses the parameters, else the number of snapshots that restored and played on to the
    uninterrupted game's record (a refused restore raises)."""
    turns = 6 if n_snapshots <= 3 else 12                        # (64 leaves need few steps per move: a longer game for 8 snapshots)
    prm = selfplay.search_params(rollouts=24 if n_snapshots <= 3 else 160, expand_thresh=3, noise_weight=0.25, sample_plies=2, max_turns=turns,
                                 record_visits=1, **kw)
    try:
        ref = selfplay.GamePool([31], prm, cap=4096, threads=1)
    except RuntimeError:
        return None
    selfplay.run_pools([ref], EV)
    # (branch_num: a game also ends where none of the policy's best moves is legal -- a root without children)
    assert ref.info(0)["done"] == 1 and (_ended(ref.moves(0), turns) or 0 < kw["branch_num"] < 81), kw
    want = (ref.moves(0), ref.info(0)["score"], [ref.visits(0, k) for k in range(len(ref.moves(0)))], ref.info(0)["n_value_evals"])
    src = selfplay.GamePool([31], prm, cap=4096, threads=1)
    blobs = []
    for step in range(100_000):
        feats, npol = src.collect()
        if len(feats) == 0:
            break
        src.deliver(*EV.finish(EV.submit(feats, npol), normalise=selfplay.normalise_rows))
        if step >= 1 and len(blobs) < n_snapshots:
            try:
                blobs.append(src.snapshot(0))
            except RuntimeError:                                  # (in the middle of a playout: simulate)
                pass
    # (a game in simulation mode is between two requests of a playout most of the time: it can be snapshotted now and then)
    assert src.moves(0) == want[0] and (len(blobs) == n_snapshots or (kw["simulate"] and blobs)), (kw, len(blobs))
    for blob in blobs:
        dst = selfplay.GamePool([1, 2], selfplay.search_params(rollouts=5, max_turns=3), cap=4096, threads=1)
        dst.restore(1, blob)                                      # ValueError: create took what restore refuses
        selfplay.run_pools([dst], EV)
        got = (dst.moves(1), dst.info(1)["score"], [dst.visits(1, k) for k in range(len(dst.moves(1)))], dst.info(1)["n_value_evals"])
        assert got == want, kw
        dst.close()
    ref.close(); src.close()
    return len(blobs)


@pytest.mark.parametrize("kw", _param_grid(), ids=lambda p: "-".join(f"{k[:2]}{v}" for k, v in p.items()))
def test_create_and_restore_agree(kw):
    """bk_pool_create either refuses a set of parameters or plays with it, and what it plays with restore takes: a snapshot taken
    after a few steps restores into a fresh pool and plays on to the uninterrupted game's record.  (leaves=100, eager=2 and a
    search with neither value net nor playouts used to play and then have every snapshot refused; a parameter out of range is
    refused by both: test_create_refuses_parameters_out_of_range.)"""
    n = _play_on_from_snapshots(kw, 8 if kw["leaves"] == 100 else 3)
    assert n is not None, kw                                     # (every point of this grid is in range: clamped or normalised, not refused)
    assert n is None or n == (8 if kw["leaves"] == 100 else 3) or (kw["simulate"] and n >= 1)


def test_create_refuses_parameters_out_of_range():
    """The ranges restore has always checked hold at create as well (one validator): a pool is not made from them."""
    for bad in (dict(rollouts=-1), dict(expand_thresh=-1), dict(c_puct=float("nan")), dict(c_puct=-1.0), dict(noise_weight=1.5), dict(max_turns=-1),
                dict(eager_top=-1), dict(branch_num=82), dict(branch_num=-1), dict(value_weight=1.5), dict(value_weight=-0.5),
                dict(komi=float("inf")), dict(speculate=-1), dict(speculate_rows=-1), dict(request_tasks=-1), dict(sample_plies=-1)):
        with pytest.raises(RuntimeError):
            selfplay.GamePool([1], selfplay.search_params(**bad), cap=256, threads=1)
    selfplay.GamePool([1], selfplay.search_params(prune=7, record_visits=-1, leaves_visit_only=9, leaves=-3, eager_top=100), cap=256, threads=1).close()   # switches: != 0


# ---- virtual loss and value_weight -----------------------------------------------------------------------------------------------
def _manual_search(**kw):
    """One manually driven game: root children's (N, V) after 60, 67 and 167 rollouts, and the pool."""
    pool = selfplay.GamePool([3], selfplay.search_params(rollouts=0, expand_thresh=6, **kw), cap=1024, threads=1)
    pool._lib.bk_pool_set_manual(pool._h, 1)
    stats = []
    for n in (60, 7, 100):
        pool._lib.bk_pool_add_rollouts(pool._h, 0, n)
        _drive(pool, "feats", 1024)
        stats.append(pool.root_children(0))
    return stats, pool


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_multi_leaf_falls_back_to_one_leaf_unless_value_weight_is_one(w):
    """virtual_loss() keeps avg = V / N, backprop ((1 - w) Q + w V) / N: with value_weight != 1 the siblings of a step would be
    compared on two scales.  Like the other modes the rule does not cover (simulate, branch_num) the search is then the one-leaf
    search; with weight 1 the mode is on (another tree).  bk_pool_set_rave and restore keep agreeing with create."""
    multi, a = _manual_search(leaves=4, value_weight=w)
    one, b = _manual_search(leaves=1, value_weight=w)
    assert multi == one and sum(n for n, _ in one[-1].values()) == 167
    on, c = _manual_search(leaves=4, value_weight=1.0)
    plain, d = _manual_search(leaves=1, value_weight=1.0)
    assert on != plain and sum(n for n, _ in on[-1].values()) == 167
    for pool, ok in ((a, False), (b, False), (c, False), (d, True)):   # RAVE: the plain backup only -- leaves = 1 AND weight 1
        if ok:
            pool.set_rave(2.0)
        else:
            with pytest.raises(ValueError):
                pool.set_rave(2.0)
    for pool in (a, b, c, d):                                          # what create made, restore takes
        dst = selfplay.GamePool([9], selfplay.search_params(rollouts=5), cap=1024, threads=1)
        dst.restore(0, pool.snapshot(0))
        assert dst.root_children(0) == pool.root_children(0)
        dst.close(); pool.close()


if __name__ == "__main__":
    rec = {f"leaves{k}": _golden_run(k, 4096) for k in (4, 8)}
    with open(GOLDEN_GAMES, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
    print("wrote", GOLDEN_GAMES, os.path.getsize(GOLDEN_GAMES), "bytes")

"""CPU: simulation balancing (bokego_amd/balance.py, bkt_balance_sums) as far as it needs no GPU -- the numpy
mirror of the kernel against a definition in Python's big integers and fractions, the invariants of the sums, the booked
share against torch autograd of the log-likelihood, the driver, the fit on the host rules, the command line, the binding and
the kernel's resources when compiled for gfx950."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import balance as B
from bokego_amd import go
from bokego_amd import lockstep as L
from bokego_amd import mmfit as MM
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from conftest import REPO

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
Q, ONE = B.Q, B.ONE
EYE_BOARD = "".join([".XXXXOOO."] + ["XXXXXOOOO"] * 3 + ["XO.XXOOOO"] + ["XXXXXOOOO"] * 3 + ["XXXXXOOO."])   # test_amaf_cpu's
SEED = 29


# ---- inputs built by hand (tests/test_gpu_balance.py runs the kernel on the same ones) -------------------------------------------
def record(game):
    return np.frombuffer(bytes(game._pos), np.uint8).reshape(1, 192).copy()


_HAND = {}


def hand_rows():
    """Six rows -> (recs uint8 [6,192], over bool [6], counters int32 [6,4]):
    0  the empty board: every point stone-free, every add of a ply collides;
    1  a record 40 plies into a uniform host-rules playout;
    2  black to move with one playable point (the capture at 38; A9 is legal but black's own eye);
    3  the same board with white to move: no playable point, the row passes and books nothing at that ply;
    4  the empty board again, already over: left alone;       5  the ply-40 record of another game."""
    if not _HAND:
        mid = RO.random_playouts(L.initial_positions(2), 5, max_plies=40, rules="host").records
        recs = np.concatenate([record(go.Game()), mid[:1], record(go.Game(EYE_BOARD)), record(go.Game(EYE_BOARD, turn=1)),
                               record(go.Game()), mid[1:]])
        _HAND["rows"] = recs, np.array([0, 0, 0, 0, 1, 0], bool), RO.default_counters(6, L.record_turns(recs))
    recs, over, ctr = _HAND["rows"]
    return recs.copy(), over.copy(), ctr.copy()


HAND_COEF = np.array([1, -1, B.MAX_COEF, -B.MAX_COEF, 7, 0], np.int64)   # 0, +-1 and both ends of the range


def table_sets():
    """name -> (patterns, tactics): tables over the whole uint16 range with entries 0 (read as 1), 1 and 65535 on the
    indices and codes the rows meet, either table missing, and both."""
    rng = np.random.default_rng(17)
    w = rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16)
    w[rng.integers(0, PT.ENTRIES, 4096)] = 0
    w[rng.integers(0, PT.ENTRIES, 4096)] = 1
    w[rng.integers(0, PT.ENTRIES, 4096)] = 65535
    w[0], w[1 << 16], w[3], w[(1 << 16) | 3] = 0, 65535, 1, 0           # the stone-free indices of the empty board's first plies
    t = rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16)
    t[8], t[4], t[9], t[20], t[0] = 65535, 0, 1, 0, 1
    small = PT.PatternTable(rng.integers(0, 4096, PT.ENTRIES).astype(np.uint16))
    return {"both": (PT.PatternTable(w), TC.TacticTable(t)), "patterns": (PT.PatternTable(w), None),
            "tactics": (None, TC.TacticTable(t)), "none": (None, None), "small": (small, TC.TacticTable.neutral())}


def random_rows(rows, seed=3):
    """Records from many plies of host-rules playouts, with the empty board at every fifth row -> (recs, counters, coef)."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([RO.random_playouts(L.initial_positions(24), 11, max_plies=k, rules="host").records for k in (3, 17, 45, 80)])
    recs = pool[rng.integers(0, len(pool), rows)]
    recs[::5] = record(go.Game())
    ctr = L.game_counters(np.arange(rows, dtype=np.uint64) + np.uint64(1000), 0, 9)
    coef = rng.integers(-B.MAX_COEF, B.MAX_COEF + 1, rows)
    coef[rng.integers(0, rows, rows // 10)] = 0
    return recs, ctr, coef


# ---- 1. the mirror against big integers ---------------------------------------------------------------------------------------
def brute(recs, over, moves, coef, patterns, tactics):
    """The definition, ply by ply over the histories `moves` on the host rules, in Python integers and fractions -> (grad_p
    dict, grad_t dict, booked plies, the sum over booked plies of 2^Q - sum_j floor(w_j 2^Q / S), the largest magnitude any
    entry reached)."""
    grad_p, grad_t, booked, slack, top = {}, {}, 0, 0, 0
    for b in range(len(recs)):
        if over[b]:
            assert (moves[b] == RO.MOVE_NONE).all()
            continue
        rec = recs[b:b + 1].copy()
        for k in range(moves.shape[1]):
            m = int(moves[b, k])
            if m == RO.MOVE_NONE:
                break
            w = [int(x) for x in RO.move_weights_host(rec, patterns, tactics)[0]]
            S = sum(w)
            assert (S == 0) == (m == go.PASS)
            if S:
                index, code = PT.codes_host(rec)[0], TC.codes_host(rec)[0]
                assert w[m] > 0
                booked += 1
                slack += ONE
                for j in range(81):
                    if w[j]:
                        share = Fraction(w[j] * ONE, S)
                        d = (ONE if j == m else 0) - share.numerator // share.denominator
                        slack -= share.numerator // share.denominator
                        for g, key in ((grad_p, int(index[j])), (grad_t, int(code[j]))):
                            g[key] = g.get(key, 0) + int(coef[b]) * d
                            top = max(top, abs(g[key]))
            L.play_host(rec, np.array([0]), np.array([m]), lambda g, mv: f"move {mv} is illegal", liberties=True)
    return grad_p, grad_t, booked, slack, top


def same_as_brute(s, want):
    grad_p, grad_t = want[:2]
    assert s.grad_p.dtype == s.grad_t.dtype == np.int64 and want[4] < 2 ** 61        # the header's bound for one call
    assert {int(i): int(s.grad_p[i]) for i in np.nonzero(s.grad_p)[0]} == {i: v for i, v in grad_p.items() if v}
    assert {int(c): int(s.grad_t[c]) for c in np.nonzero(s.grad_t)[0]} == {c: v for c, v in grad_t.items() if v}


@pytest.mark.parametrize("name", ["both", "patterns", "tactics", "none"])
@pytest.mark.parametrize("max_plies", [1, 8, 60])
def test_the_mirror_equals_big_integer_arithmetic(name, max_plies):
    patterns, tactics = table_sets()[name]
    recs, over, ctr = hand_rows()
    s = B.sums_host(recs, SEED, ctr, HAND_COEF, patterns, tactics, max_plies, over=over)
    # the games are random_playouts' games: the wrapper reads, it never changes a draw
    live = ~over
    fin = RO.random_playouts(recs[live], SEED, ctr[live], max_plies, rules="host", patterns=patterns, tactics=tactics)
    assert np.array_equal(s.moves[live][:, :fin.moves.shape[1]], fin.moves) and (s.moves[live][:, fin.moves.shape[1]:] == RO.MOVE_NONE).all()
    assert np.array_equal(s.records[live], fin.records) and np.array_equal(s.over[live], fin.over) and np.array_equal(s.plies[live], fin.plies)
    assert np.array_equal(s.records[over], recs[over]) and s.over[over].all() and (s.plies[over] == 0).all()
    want = brute(recs, over, s.moves, HAND_COEF, patterns, tactics)
    same_as_brute(s, want)
    assert s.moves[3, 0] == go.PASS and (max_plies == 1 or s.moves[3, 1] == 38)     # the row with no playable point passes
    assert s.moves[2, 0] == 38                                                       # the row with one plays it
    if max_plies == 60:
        assert s.plies.max() == 60 and not s.over[0]                                 # the cap cuts the empty board's game short
    assert want[2] > 0 and (s.grad_p.any() and s.grad_t.any())


# ---- 2. invariants ---------------------------------------------------------------------------------------------------------------
def test_invariants_of_the_sums():
    patterns, tactics = table_sets()["both"]
    recs, over, ctr = hand_rows()
    ones = np.ones(6, np.int64)
    s = B.sums_host(recs, SEED, ctr, ones, patterns, tactics, 24, over=over)
    _, _, booked, slack, _ = brute(recs, over, s.moves, ones, patterns, tactics)
    assert s.grad_p.sum() == s.grad_t.sum() == slack and 0 <= slack <= 81 * booked   # floors of 81 shares that sum to 1
    # rows with coef 0 change nothing, and the other rows do not depend on them
    c = HAND_COEF.copy()
    c[[1, 2]] = 0
    a = B.sums_host(recs, SEED, ctr, c, patterns, tactics, 24, over=over)
    keep = np.array([0, 3, 4, 5])
    b = B.sums_host(recs[keep], SEED, ctr[keep], c[keep], patterns, tactics, 24, over=over[keep])
    assert np.array_equal(a.grad_p, b.grad_p) and np.array_equal(a.grad_t, b.grad_t) and a.grad_t.any()
    assert np.array_equal(a.moves, s.moves)                                          # ... nor do the games depend on coef
    zero = B.sums_host(recs, SEED, ctr, 0 * ones, patterns, tactics, 24, over=over)
    assert not zero.grad_p.any() and not zero.grad_t.any()
    # two calls over split rows equal one call; coef -> -coef negates the sums exactly
    whole = B.sums_host(recs, SEED, ctr, HAND_COEF, patterns, tactics, 24, over=over)
    first, second = (B.sums_host(recs[p], SEED, ctr[p], HAND_COEF[p], patterns, tactics, 24, over=over[p]) for p in (slice(0, 2), slice(2, 6)))
    assert np.array_equal(first.grad_p + second.grad_p, whole.grad_p) and np.array_equal(first.grad_t + second.grad_t, whole.grad_t)
    neg = B.sums_host(recs, SEED, ctr, -HAND_COEF, patterns, tactics, 24, over=over)
    assert np.array_equal(neg.grad_p, -whole.grad_p) and np.array_equal(neg.grad_t, -whole.grad_t) and whole.grad_p.any()


# ---- 3. the booked share is the gradient of log pi ------------------------------------------------------------------------------
def test_the_sums_are_the_gradient_of_the_log_likelihood():
    """Three host-rules games of 20 plies.  Pattern entries 16..4095 and tactics entries 256 k, k = 1..8: w = (P * 256 k) >> 8 =
    P k exactly, at least 16 and below 2^16, so neither max(1, .) nor the shift nor uint16 touches a weight and w is
    exp(theta_p + theta_t) / 256 in real numbers."""
    rng = np.random.default_rng(5)
    patterns = PT.PatternTable(rng.integers(16, 4096, PT.ENTRIES).astype(np.uint16))
    tactics = TC.TacticTable((256 * rng.integers(1, 9, TC.ENTRIES)).astype(np.uint16))
    start = L.initial_positions(3)
    ctr = RO.default_counters(3, L.record_turns(start))
    s = B.sums_host(start, 8, ctr, np.ones(3, np.int64), patterns, tactics, 20)
    theta_p = torch.tensor(np.log(patterns.array.astype(np.float64)), requires_grad=True)
    theta_t = torch.tensor(np.log(tactics.array.astype(np.float64)), requires_grad=True)
    ll, booked = 0.0, 0
    for g in range(3):
        rec = start[g:g + 1].copy()
        for k in range(20):
            m = int(s.moves[g, k])
            ok = torch.from_numpy(RO.playable_host(rec)[0])
            assert ok.any() and m >= 0                                   # 20 plies from the empty board: nobody passes
            index = torch.from_numpy(PT.codes_host(rec)[0].astype(np.int64))
            code = torch.from_numpy(TC.codes_host(rec)[0].astype(np.int64))
            logw = (theta_p[index] + theta_t[code])[ok]
            ll = ll + (theta_p[index[m]] + theta_t[code[m]]) - torch.logsumexp(logw, 0)
            booked += 1
            L.play_host(rec, np.array([0]), np.array([m]), lambda g_, mv: f"move {mv} is illegal", liberties=True)
    ll.backward()
    # Allowance.  An entry collects at most one term per candidate and ply, booked * 81 of them.  The integer side floors
    # each share to a multiple of 2^-Q: below the real share by less than 2^-Q a term.  The float64 side: a share is
    # exp(x - logsumexp) with x and the 81-term logsumexp each good to a few ulp of values below 32 (log 2^16 * 2 = 22), so
    # a share in [0, 1] carries an absolute error below 128 * 2^-53 * 32 = 2^-41; the backward pass adds the terms with
    # one rounding each of a partial sum that is at most `booked`.
    allowance = booked * 81 * 2.0 ** -Q + booked * 81 * (2.0 ** -41 + booked * 2.0 ** -53)
    for name, got, want in (("patterns", s.grad_p, theta_p.grad.numpy()), ("tactics", s.grad_t, theta_t.grad.numpy())):
        diff = got.astype(np.float64) / ONE - want
        print(name, "largest difference", float(np.abs(diff).max()), "allowed", allowance)
        assert (np.abs(diff) <= allowance).all() and np.abs(want).max() > 0.5
        assert (diff >= -booked * 81 * (2.0 ** -41 + booked * 2.0 ** -53)).all()   # a floored share only raises d = hit - share


# ---- 4. the driver ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def positions():
    """Eight positions 30 plies into uniform host-rules playouts, and targets over [-1, 1]."""
    recs = RO.random_playouts(L.initial_positions(8), 3, max_plies=30, rules="host").records
    return recs, np.array([1.0, -1.0, 0.5, -0.25, 0.0, 1.0, -1.0, 0.3])


def test_the_coefficients_by_hand():
    D, coef = B.coefficients([1.0, -1.0, 0.3, 0.5], [4, 4, 0, 1], [[1, 0], [0, 0], [1, 1], [0, 1]], M=4)
    # V* M rounds to 4, -4, 1 (1.2), 2; 2 wins - M = 4, 4, -4, -2
    assert D.tolist() == [0, -8, 5, 4] and coef.tolist() == [[0, 0], [8, 8], [5, 5], [-4, 4]]
    assert B.coefficients([0.125], [2], [[1]], M=4)[0].tolist() == [0]               # rint: 0.5 goes to the even 0


def test_gradient_is_its_three_runs(positions):
    recs, targets = positions
    patterns, tactics = table_sets()["small"]
    M, N, seed = 4, 3, 12
    g = B.gradient(recs, targets, patterns, tactics, M, N, seed, rules="host")
    V = RO.playout_value(recs, M, seed, rules="host", patterns=patterns, tactics=tactics).astype(np.float64)
    wins = np.rint((V * M + M) / 2).astype(np.int64)
    assert np.array_equal(g.wins, wins) and g.mse == pytest.approx(np.mean((targets - V) ** 2)) and g.norm == M * N * 8 * ONE
    D = np.rint(targets * M).astype(np.int64) - (2 * wins - M)
    assert np.array_equal(g.D, D) and np.abs(D).max() <= 2 * M and D.any()
    key_b = (seed + B.KEY_STEP) % 2 ** 64
    second = RO._playouts(recs, N, key_b, "host", table=patterns, tactics=tactics)
    coef = np.where(second.won, 1, -1) * D[:, None]
    s = B.sums_host(np.repeat(recs, N, 0), key_b, RO.value_counters(recs, N), coef.reshape(-1), patterns, tactics)
    assert np.array_equal(g.grad_p, s.grad_p) and np.array_equal(g.grad_t, s.grad_t) and g.grad_t.any()
    first = RO._playouts(recs, M, seed, "host", table=patterns, tactics=tactics, max_plies=50, history=True)
    assert not np.array_equal(first.moves[:N], s.moves[:N, :first.moves.shape[1]])   # two independent sets
    for bad in (dict(targets=targets * 2), dict(targets=targets[:-1]), dict(M=B.MAX_COEF), dict(N=0), dict(rules="gnugo"),
                dict(max_plies=0)):
        with pytest.raises(ValueError):
            B.gradient(**{**dict(positions=recs, targets=targets, M=M, N=N, seed=seed, rules="host"), **bad})


def test_two_fits_give_the_same_bits_and_tables_that_play(positions):
    recs, targets = positions
    kw = dict(iterations=2, lr=4.0, M=4, N=3, rules="host", seed=2, max_plies=50, held_out=(recs[:3], targets[:3]))
    a, b = B.fit(recs, targets, **kw), B.fit(recs.copy(), targets.copy(), **kw)
    assert np.array_equal(a.gp, b.gp) and np.array_equal(a.gt, b.gt) and a.log == b.log
    assert a.gp.dtype == a.gt.dtype == np.uint32 and (a.gt != MM.G_ONE).any() and (a.gp != MM.G_ONE).any()
    assert np.array_equal(a.gp, a.gp[PT._canonical()])                               # equal strengths over every orbit
    assert [r["iteration"] for r in a.log] == [0, 1, 2] and a.log[2]["mse"] is None and a.log[0]["mse"] > 0
    assert all(0 <= r["held_out_agreement"] <= 1 and r["held_out_mse"] >= 0 for r in a.log)
    assert isinstance(a.patterns, PT.PatternTable) and isinstance(a.tactics, TC.TacticTable)
    want = MM.tables(a.gp, a.gt)
    assert np.array_equal(a.patterns.array, want[0].array) and np.array_equal(a.tactics.array, want[1].array)
    fin = RO.random_playouts(L.initial_positions(2), 9, max_plies=30, rules="host", patterns=a.patterns, tactics=a.tactics)
    assert fin.moves.shape == (2, 30) and (fin.moves >= -1).all()
    # the first step by hand: theta = lr * pooled(grad) / norm from gamma = 1
    g = B.gradient(recs, targets, *MM.tables(*B.strengths_of_tables()), 4, 3, 2, rules="host", max_plies=50)
    one = B.fit(recs, targets, iterations=1, lr=4.0, M=4, N=3, rules="host", seed=2, max_plies=50)
    theta = 4.0 * MM.pooled(MM.GROUPS[1], g.grad_t).astype(np.float64) / g.norm
    assert np.array_equal(one.gt, np.clip(np.rint(np.exp(theta) * MM.G_ONE), MM.G_MIN, MM.G_MAX).astype(np.uint32))
    # weight decay pulls towards the start, a given start is where the fit begins
    start = B.strengths_of_tables(*table_sets()["small"])
    assert np.array_equal(MM.tables(*start)[0].array, np.maximum(table_sets()["small"][0].array, 1))
    zero = B.fit(recs, targets, iterations=0, start=start, rules="host")
    assert np.array_equal(zero.gp, start[0]) and np.array_equal(zero.gt, start[1]) and len(zero.log) == 1
    for bad in (dict(iterations=-1), dict(lr=0), dict(prior=-1), dict(rules="gnugo")):
        with pytest.raises(ValueError):
            B.fit(recs, targets, **{**dict(rules="host"), **bad})


def test_labelled_positions_and_the_value_error():
    start = L.initial_positions(4)
    fin = RO.random_playouts(start, 6, max_plies=300, rules="host")
    pos, tgt, game, ply = B.labelled_positions(start, fin.moves, plies=(0, 10))
    assert pos.shape == (8, 192) and game.tolist() == [0, 1, 2, 3] * 2 and ply.tolist() == [0] * 4 + [10] * 4
    assert np.array_equal(pos[:4], start) and (L.record_turns(pos[4:]) == 10).all()
    black_won = fin.score > 0
    assert np.array_equal(tgt, np.where(np.tile(black_won, 2), 1.0, -1.0))           # black is to move at plies 0 and 10
    odd = B.labelled_positions(start, fin.moves, plies=(7,))
    assert np.array_equal(odd[1], np.where(black_won, -1.0, 1.0))
    assert len(B.labelled_positions(start, fin.moves, plies=(1000,))[0]) == 0
    e = B.value_error(pos, tgt, n=8, seed=1, rules="host")
    v = RO.playout_value(pos, 8, 1, rules="host").astype(np.float64)
    assert e["positions"] == 8 and e["mse"] == pytest.approx(np.mean((tgt - v) ** 2))
    assert e["agreement"] == pytest.approx(np.mean(((v > 0) == (tgt > 0)) & (v != 0))) and e["ties"] == np.mean(v == 0)


# ---- 5. the interface ------------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    out = ["--patterns-out", "p.npy", "--tactics-out", "t.npy"]
    a = B.parse_args(["fit", "-p", "w.bkw"] + out)
    assert (a.games, a.seed, a.records, a.plies, a.iterations, a.lr, a.playouts, a.samples, a.prior, a.scale) == \
        (4096, 0, None, [40], 20, 1.0, 64, 64, 0.0, 64) and a.start_patterns is None and a.start_tactics is None
    a = B.parse_args(["fit", "--games", "0", "--records", "a", "b", "--plies", "20", "40", "--iterations", "5", "--lr", "0.5",
                      "--playouts", "32", "--samples", "16", "--prior", "0.1", "--start-patterns", "sp.npy", "--start-tactics",
                      "st.npy"] + out)
    assert (a.p, a.games, a.records, a.plies, a.iterations, a.lr, a.playouts, a.samples, a.prior) == \
        (None, 0, ["a", "b"], [20, 40], 5, 0.5, 32, 16, 0.1) and (a.start_patterns, a.start_tactics) == ("sp.npy", "st.npy")
    a = B.parse_args(["eval", "--patterns", "p.npy", "--tactics", "t.npy", "-p", "w.bkw", "--games", "8", "--seed", "3"])
    assert (a.command, a.patterns, a.tactics, a.games, a.seed, a.plies, a.playouts) == ("eval", "p.npy", "t.npy", 8, 3, [40], 64)
    for bad in (["fit", "-p", "w"], ["fit", "-p", "w", "--games", "0"] + out, ["fit", "--games", "4"] + out,
                ["fit", "-p", "w", "--iterations", "0"] + out, ["fit", "-p", "w", "--lr", "0"] + out,
                ["fit", "-p", "w", "--playouts", str(B.MAX_COEF)] + out, ["fit", "-p", "w", "--samples", "0"] + out,
                ["fit", "-p", "w", "--prior", "-1"] + out, ["fit", "-p", "w", "--scale", "0"] + out,
                ["fit", "-p", "w", "--plies", "-1"] + out, ["fit", "-p", "w", "--seed", "-1"] + out,
                ["eval", "--games", "8"], ["eval", "-p", "w", "--games", "0"], []):
        with pytest.raises(SystemExit):
            B.parse_args(bad)
    capsys.readouterr()


def test_coefficients_outside_the_range_are_refused():
    recs, over, ctr = hand_rows()
    assert T.balance_coef(HAND_COEF, 6).dtype == torch.int32 and T.balance_coef(HAND_COEF, 6).tolist() == HAND_COEF.tolist()
    for value in (B.MAX_COEF + 1, -B.MAX_COEF - 1, 2 ** 31):
        bad = HAND_COEF.copy()
        bad[3] = value
        with pytest.raises(ValueError, match="coefficient"):
            T.balance_coef(bad, 6)
        with pytest.raises(ValueError, match="coefficient"):
            B.sums_host(recs, SEED, ctr, bad, None, None, 4)
    for bad in (HAND_COEF[:-1], HAND_COEF.astype(np.float64), HAND_COEF.reshape(2, 3)):
        with pytest.raises(ValueError):
            T.balance_coef(bad, 6)
        with pytest.raises(ValueError):
            B.sums_host(recs, SEED, ctr, bad, None, None, 4)
    for max_plies in (0, 1025):
        with pytest.raises(ValueError):
            B.sums_host(recs, SEED, ctr, HAND_COEF, None, None, max_plies)
    with pytest.raises(ValueError):
        B.sums_host(recs, SEED, ctr[:-1], HAND_COEF, None, None, 4)
    with pytest.raises(ValueError):
        B.sums(recs, SEED, ctr, HAND_COEF, rules="gnugo")
    assert (T.BALANCE_Q, T.BALANCE_MAX_ROWS, T.BALANCE_MAX_COEF) == (24, 16384, 4096)
    assert T.BALANCE_MAX_COEF * 2 ** (T.BALANCE_Q + 1) * T.MAX_PLAYOUT_PLIES * T.BALANCE_MAX_ROWS == 2 ** 61   # the header's bound


def test_header_binding_and_library_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_balance_sums\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,\s*const\s+uint16_t\s*\*\s*tactics\s*,"
                     r"\s*const\s+int32_t\s*\*\s*coef\s*,\s*int64_t\s*\*\s*grad_p\s*,\s*int64_t\s*\*\s*grad_t\s*,\s*int\s+max_plies\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,\s*int32_t\s*\*\s*status\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    for name, value in (("BKT_BALANCE_Q", 24), ("BKT_BALANCE_MAX_ROWS", 16384), ("BKT_BALANCE_MAX_COEF", 4096)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src)
    res, args = T.SYMBOLS["bkt_balance_sums"]
    P, I, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert res is I and args == [P, I, U64, P, P, P, P, P, P, I, P, P, P, P, P] and callable(T.balance_sums)
    assert all(hasattr(B, name) for name in B.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_balance_sums
    # the Makefile: a dependency of the library's rule, not a source on its compile line; included as text in the chain
    make = open(os.path.join(CSRC, "Makefile")).read()
    rule, line = re.search(r"^\$\(TRAIN_OUT\):(.*)\n\t(.*)$", make, flags=re.M).groups()
    assert "bk_playout_balance.hip" in rule.split() and "bk_playout_balance.hip" not in line
    pat = open(os.path.join(CSRC, "bk_playout_pat.hip")).read()
    assert pat.index('#include "bk_playout_reply.hip"') < pat.index('#include "bk_playout_balance.hip"')
    for name in ("bk_playout.hip", "bk_playout_mc.hip", "bk_playout_tac.hip", "bk_playout_reply.hip", "bk_playout_reply2.hip",
                 "bk_playout_reply2_tables.hip", "bk_playout_mm.hip"):
        assert "balance" not in open(os.path.join(CSRC, name)).read()
    own = open(os.path.join(CSRC, "bk_playout_balance.hip")).read()
    assert "float" not in own and "double" not in own and "BalanceDraw<WeightedDraw<OptionalTacticalWeight>>" in own
    assert own.count("__syncthreads") == 1                              # the one before the flush, behind the ply loop
    assert not re.search(r"#include", own.split("namespace {")[0].replace("included as text", ""))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_has_no_spills_or_scratch_and_the_wrapped_kernel_keeps_its_resources(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]

    def fields(name):
        (block,) = [b for b in blocks if re.search(r"\d" + name + "E", b.split()[0])]
        return {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in
                (("occupancy", r"Occupancy \[waves/SIMD\]"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                 ("sspill", r"SGPRs Spill"), ("vspill", r"VGPRs Spill"), ("lds", r"LDS Size \[bytes/block\]"),
                 ("vgprs", r" VGPRs"))}

    f, tactical = fields("balance_sums_kernel"), fields("tactical_playouts_kernel")
    assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, f
    # 512 stone-free indices and 64 codes as 64-bit sums, and the two accumulators' addresses
    assert f["lds"] == tactical["lds"] + 512 * 8 + 64 * 8 + 2 * 8, (f, tactical)
    assert f["vgprs"] <= 128 and f["occupancy"] >= 4, f
    assert tactical["scratch"] == 0 and tactical["sspill"] == 0 and tactical["vspill"] == 0 and tactical["occupancy"] >= 4

"""CPU: the joint MM fit of the pattern and the tactics table (bokego_amd/mmfit.py, bkt_mm_sums) as far as it
needs no GPU -- the numpy mirror of the kernel against Python's big integers, the tie to tactics.counts, the fit on the host
rules, the rows that must add nothing, the command line, the binding and the kernel's resources when compiled for gfx950."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import go
from bokego_amd import lockstep as L
from bokego_amd import mmfit as M
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from conftest import REPO

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
G_MIN, G_MAX, ONE = M.G_MIN, M.G_MAX, M.G_ONE
NEAR = 1 << 16


# ---- inputs built by hand (tests/test_gpu_mmfit.py runs the kernel on the same ones) ---------------------------------------------
def word(index, code, playable=True):
    return int(index) | int(code) << 17 | (1 << 31 if playable else 0)


def random_rows(rng, rows, indices=40, p_playable=0.6):
    """Rows over a few indices (both halves of the table) and all codes, so that the adds of a row collide."""
    pool = np.concatenate([rng.integers(0, NEAR, indices // 2), NEAR + rng.integers(0, NEAR, indices // 2), [0, NEAR, 0xFFFF]])
    index = pool[rng.integers(0, len(pool), (rows, 81))]
    code = rng.integers(0, 64, (rows, 81))
    codes = M.pack_word(index, code, rng.random((rows, 81)) < p_playable)
    return codes, rng.integers(-2, 81, rows).astype(np.int32)


def hand_rows():
    """Seven rows -> (codes uint32 [7,81], moves int32 [7]):
    0  all 81 points playable on index 0 and code 8, the move in the middle: every add collides, every strength ties;
    1  one playable point, and it is played;             2  no playable point, a point "played";
    3  a played point that is not playable;             4  a pass;             5  MOVE_NONE;
    6  indices in the `near` half, and the played word repeated before and after the move: rank's tie rule."""
    rng = np.random.default_rng(28)
    codes, moves = random_rows(rng, 7)
    codes[0], moves[0] = word(0, 8), 40
    codes[1] = codes[1] & np.uint32(0x7FFFFFFF)
    codes[1, 17], moves[1] = word(NEAR | 0x1234, 9), 17
    codes[2], moves[2] = codes[2] & np.uint32(0x7FFFFFFF), 5
    codes[3, 30], moves[3] = word(0x0042, 3, playable=False), 30
    moves[4], moves[5] = -1, -2
    codes[6] = M.pack_word(NEAR | (codes[6] & np.uint32(0xFFFF)), (codes[6] >> np.uint32(17)) & np.uint32(63), True)
    codes[6, [3, 20, 41, 44, 70]], moves[6] = word(NEAR | 0x0F0F, 21), 41
    return codes, moves


def strengths(rng, kind="random"):
    """(gp, gt) uint32: random over the whole domain with entries at both of its ends, or one of its corners."""
    if kind == "random":
        gp = (2.0 ** rng.uniform(8, 24, PT.ENTRIES)).astype(np.uint32)
        gt = (2.0 ** rng.uniform(8, 24, TC.ENTRIES)).astype(np.uint32)
        gp[rng.integers(0, PT.ENTRIES, 20000)], gp[rng.integers(0, PT.ENTRIES, 20000)] = G_MIN, G_MAX
        gp[0], gp[NEAR], gp[NEAR | 0x0F0F], gp[NEAR | 0x1234] = G_MAX, G_MIN, G_MIN, G_MAX
        gt[[8, 21, 3]], gt[[9, 63, 0]] = G_MIN, G_MAX
        return gp, gt
    p, t = {"low": (G_MIN, G_MIN), "high": (G_MAX, G_MAX), "low-high": (G_MIN, G_MAX), "high-low": (G_MAX, G_MIN)}[kind]
    return np.full(PT.ENTRIES, p, np.uint32), np.full(TC.ENTRIES, t, np.uint32)


def brute(codes, moves, gp, gt):
    """bkt_mm_sums' definition in Python integers of any size -> the five results as lists / dicts, and the largest value
    any step produced."""
    den_p, den_t, total, chosen, rank, top = {}, {}, [], [], [], 0
    for r in range(len(codes)):
        pts = [(j, int(codes[r, j]) & 0x1FFFF, int(codes[r, j]) >> 17 & 63) for j in range(81) if int(codes[r, j]) >> 31]
        s = {j: max(1, int(gp[i]) * int(gt[c]) >> 16) for j, i, c in pts}
        E, m = sum(s.values()), int(moves[r])
        total.append(E)
        top = max(top, E)
        if m in s:
            chosen.append(s[m])
            rank.append(sum(1 for j in s if s[j] > s[m] or (s[j] == s[m] and j < m)))
            for j, i, c in pts:
                den_p[i] = den_p.get(i, 0) + (int(gt[c]) << 32) // E
                den_t[c] = den_t.get(c, 0) + (int(gp[i]) << 32) // E
                top = max(top, int(gt[c]) << 32, int(gp[i]) << 32, int(gp[i]) * int(gt[c]))
        else:
            chosen.append(0)
            rank.append(-1)
    return den_p, den_t, total, chosen, rank, max([top] + list(den_p.values()) + list(den_t.values()))


def same_as_brute(s, want):
    den_p, den_t, total, chosen, rank, top = want
    assert top < 2 ** 64                                              # no value wraps
    assert s.den_p.dtype == s.den_t.dtype == s.total.dtype == s.chosen.dtype == np.uint64 and s.rank.dtype == np.int32
    assert [int(x) for x in s.total] == total and [int(x) for x in s.chosen] == chosen and s.rank.tolist() == rank
    assert {int(i): int(s.den_p[i]) for i in np.nonzero(s.den_p)[0]} == {i: v for i, v in den_p.items() if v}
    assert {int(c): int(s.den_t[c]) for c in np.nonzero(s.den_t)[0]} == {c: v for c, v in den_t.items() if v}


# ---- 1. the mirror against big integers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "low", "high", "low-high", "high-low"])
def test_the_mirror_equals_big_integer_arithmetic(kind):
    rng = np.random.default_rng(1)
    gp, gt = strengths(rng, kind)
    for codes, moves in (hand_rows(), random_rows(rng, 12), random_rows(rng, 5, indices=2, p_playable=1.0)):
        same_as_brute(M.sums_host(codes, moves, gp, gt), brute(codes, moves, gp, gt))


@pytest.mark.parametrize("kind", ["low", "high", "low-high", "high-low"])
def test_a_full_call_of_identical_rows_at_the_corners(kind):
    """T.MM_MAX_ROWS rows, each 81 playable points on one index and one code: every value is known in closed form, and the
    sums are the largest a call can make of that corner."""
    gp, gt = strengths(None, kind)
    R = T.MM_MAX_ROWS
    codes = np.full((R, 81), word(5, 7), np.uint32)
    s = M.sums_host(codes, np.full(R, 80, np.int32), gp, gt)
    p, t = int(gp[0]), int(gt[0])
    one = max(1, p * t >> 16)
    E = 81 * one
    assert (s.total == E).all() and (s.chosen == one).all() and (s.rank == 80).all()
    want_p, want_t = R * 81 * ((t << 32) // E), R * 81 * ((p << 32) // E)
    assert max(want_p, want_t) < 2 ** 55                               # the header's bound for one call
    assert int(s.den_p[5]) == want_p and int(s.den_t[7]) == want_t and s.den_p.sum() == s.den_p[5] and s.den_t.sum() == s.den_t[7]


# ---- 2. the tie to the tested fit ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def games():
    """Six host-rule games of 40 plies from the empty board (uniform playouts), and a pattern table over many values."""
    start = L.initial_positions(6)
    fin = RO.random_playouts(start, 5, max_plies=40, rules="host")
    table = PT.PatternTable(np.random.default_rng(3).integers(0, 4096, PT.ENTRIES).astype(np.uint16))
    return start, fin.moves, table


def test_den_t_is_the_mass_of_tactics_counts(games):
    start, moves, table = games
    d = M.pack(start, moves, rules="host")
    mass, played = TC.counts(start, moves, table, rules="host")
    assert np.array_equal(d.played_t, played)
    assert np.array_equal(d.played_p, PT.counts(start, moves, rules="host")[1])
    gp = np.maximum(table.array.astype(np.uint32), 1) << 8
    s = M.sums_host(d.codes, d.moves, gp, np.full(TC.ENTRIES, ONE, np.uint32))
    valid = s.rank >= 0                                                # the plies tactics.counts counts
    assert valid.all() and valid.sum() == played.sum()                 # a playout plays playable points only
    # with gt = 1, s_j = gp >> 0 = P << 8 exactly, so a term is floor(2^32 P / sum P): below the float64 share by < 2^-32
    # mass's own float64 sum: rows * 81 additions, each rounding a partial sum that is at most `rows`
    rows = int(valid.sum())
    own = rows * 81 * rows * 2.0 ** -53
    diff = mass - s.den_t.astype(np.float64) / 2.0 ** 32
    assert (diff >= -own).all() and (diff <= rows * 81 * 2.0 ** -32 + own).all(), (diff.min(), diff.max())


# ---- 3. the fit ----------------------------------------------------------------------------------------------------------------
def rounding_allowance(gp, gt):
    """The relative change one rounding of the format can make in a candidate's strength s = (gp gt) >> 16: half a unit of
    either g, and the unit the shift drops from s.  From the format alone: g >= min g, s >= (min gp)(min gt) >> 16."""
    lo_p, lo_t = int(np.min(gp)), int(np.min(gt))
    return 0.5 / lo_p + 0.5 / lo_t + 1.0 / max(1, lo_p * lo_t >> 16)


@pytest.fixture(scope="module")
def small_fit():
    """Three games of 16 plies, 400 iterations: the iteration is linear and its slowest direction is the common scale of the
    two groups, which only the prior holds."""
    start = L.initial_positions(3)
    fin = RO.random_playouts(start, 5, max_plies=16, rules="host")
    data = M.pack(start, fin.moves, rules="host")
    return start, fin.moves, data, M.fit(data, iterations=400, prior=1.0, rules="host")


def test_the_fit_never_loses_likelihood_and_ends_at_a_fixed_point(small_fit):
    start, moves, data, f = small_fit
    assert len(f.log) == 801 and f.log[0]["updated"] == "patterns" and f.log[1]["updated"] == "tactics" and f.log[-1]["updated"] is None
    n = f.log[0]["moves"]
    assert n == int(data.played_t.sum()) > 40
    assert f.log[0]["mean_ll"] == pytest.approx(np.mean(-np.log(M.sums(data, *[np.full(g.entries, ONE) for g in M.GROUPS],
                                                                       rules="host").total.astype(float) / ONE)))
    # Monotone.  In real numbers an MM step never lowers the penalised likelihood.  The logged value is the integer model's:
    # each of the n moves enters as log s_m - log E, and each of those two terms moves by at most the allowance when the
    # step's result is rounded into the format (before and after the step: twice); the prior's term a log g - 2a log(g+1)
    # of a feature moves by at most 3a times the allowance -- of a feature that moves at all: one that is no candidate
    # anywhere in the data stays at gamma = 1 exactly, which the format holds without rounding.
    eps = rounding_allowance(f.gp, f.gt)
    index = (data.codes & np.uint32(PT.ENTRIES - 1))[(data.codes >> np.uint32(31)) != 0]
    features = len(np.unique(PT._canonical()[index])) + TC.ENTRIES
    slack = 2 * (2 * n * eps) + 3 * 1.0 * features * eps
    ll = np.array([row["penalised_ll"] for row in f.log])
    print("largest loss of a half-iteration", float(-np.diff(ll).min()), "allowed", slack)
    assert (np.diff(ll) >= -slack).all()
    assert ll[-1] > ll[0] + 10 and f.log[-1]["top1"] > f.log[0]["top1"]
    # The fixed point: gamma (D + 2a / (gamma + 1)) = W + a, D from a pass over the final tables.  Both factors carry one
    # rounding: gamma its own, D that of every strength in it.
    s = M.sums(data, f.gp, f.gt, rules="host")
    for group, g, W, den in zip(M.GROUPS, (f.gp, f.gt), (data.played_p, data.played_t), (s.den_p, s.den_t)):
        gamma = g / ONE
        W, D = M.pooled(group, W).astype(np.float64), M.pooled(group, den).astype(np.float64) / 2.0 ** 32
        check = (W > 0) & (g > G_MIN) & (g < G_MAX)
        assert check.sum() >= 3
        miss = np.abs(gamma * (D + 2.0 / (gamma + 1)) - (W + 1))[check]
        print(group.name, "largest miss / allowance", float((miss / (2 * eps * (W[check] + 1))).max()))
        assert (miss <= 2 * eps * (W[check] + 1)).all()
    # every index of a dihedral orbit has the same strength; a feature never seen went towards 1
    assert np.array_equal(f.gp, f.gp[PT._canonical()])
    unseen = M.pooled(M.GROUPS[0], s.den_p) == 0
    assert unseen.any() and (f.gp[unseen] == ONE).all()


def test_two_fits_give_the_same_bits_and_tables_that_play(small_fit):
    start, moves, data, f = small_fit
    a, b = M.fit(data, iterations=3, rules="host"), M.fit(M.pack(start, moves, rules="host"), iterations=3, rules="host")
    assert np.array_equal(a.gp, b.gp) and np.array_equal(a.gt, b.gt) and a.log == b.log
    assert a.gp.dtype == a.gt.dtype == np.uint32 and not np.array_equal(a.gt, f.gt)
    table, tactics = M.tables(f.gp, f.gt)
    assert isinstance(table, PT.PatternTable) and isinstance(tactics, TC.TacticTable)
    assert np.array_equal(table.array, np.clip(np.floor(64 * f.gp / ONE + 0.5), 1, 65535).astype(np.uint16))
    assert np.array_equal(tactics.array, np.clip(np.floor(256 * f.gt / ONE + 0.5), 1, 65535).astype(np.uint16))
    top, _ = M.tables(np.full(PT.ENTRIES, G_MAX), np.full(TC.ENTRIES, G_MIN))
    assert (top.array == 16384).all() and (_.array == 1).all()        # the whole domain fits without clipping at the top
    fin = RO.random_playouts(L.initial_positions(2), 9, max_plies=30, rules="host", patterns=table, tactics=tactics)
    assert fin.moves.shape == (2, 30) and (fin.moves >= -1).all()
    assert not np.array_equal(fin.moves, RO.random_playouts(L.initial_positions(2), 9, max_plies=30, rules="host").moves)
    # the fitted pair predicts the games it was fitted on better than no tables, under the draw itself
    fitted, uniform = M.evaluate(start, moves, table, tactics, rules="host"), M.evaluate(start, moves, rules="host")
    assert fitted["moves"] == uniform["moves"] == f.log[0]["moves"]
    assert uniform["mean_ll"] == pytest.approx(f.log[0]["mean_ll"]) and fitted["mean_ll"] > uniform["mean_ll"] + 0.2
    print("mean log-likelihood: strengths", f.log[-1]["mean_ll"], "tables", fitted["mean_ll"])   # what the rounding costs
    assert M.evaluate(start, moves, table, tactics, rules="host", plies=[0, 7])["moves"] == 6
    for bad in (dict(iterations=-1), dict(prior=0), dict(prior=float("nan")), dict(rules="gnugo")):
        with pytest.raises(ValueError):
            M.fit(data, **{"rules": "host", **bad})
    with pytest.raises(ValueError):
        M.tables(f.gp, f.gt, scale=0)


# ---- 4. rows that must add nothing -----------------------------------------------------------------------------------------------
EYE_BOARD = "".join([".XXXXOOO."] + ["XXXXXOOOO"] * 3 + ["XO.XXOOOO"] + ["XXXXXOOOO"] * 3 + ["XXXXXOOO."])   # test_amaf_cpu's


def test_rows_that_add_nothing():
    # black fills its own eye at A9 (point 0: legal, not playable), white passes, black captures at 38, both pass
    start = np.frombuffer(bytes(go.Game(EYE_BOARD)._pos), np.uint8).reshape(1, 192).copy()
    moves = np.array([[0, -1, 38, -1, -1, -2, -2]], np.int32)
    d = M.pack(start, moves, rules="host")
    assert d.codes.shape == (5, 81) and d.moves.tolist() == [0, -1, 38, -1, -1]            # MOVE_NONE plies have no row
    assert d.played_t.sum() == d.played_p.sum() == 1                                        # only the capture counts
    playable = (d.codes >> np.uint32(31)).astype(bool)
    assert playable[0].sum() == 1 and not playable[0, 0] and playable[0, 38]              # the eye is legal, not playable
    s = M.sums_host(d.codes, d.moves, *strengths(np.random.default_rng(4)))
    assert s.rank.tolist() == [-1, -1, 0, -1, -1] and s.chosen[[0, 1, 3, 4]].tolist() == [0] * 4 and s.chosen[2] == s.total[2] > 0
    assert s.total[0] > 0
    none = playable.sum(1) == 0
    assert none.any() and (s.total[none] == 0).all()                                        # rows with no playable point
    only = M.sums_host(d.codes[2:3], d.moves[2:3], *strengths(np.random.default_rng(4)))
    assert np.array_equal(only.den_p, s.den_p) and np.array_equal(only.den_t, s.den_t) and s.den_t.sum() > 0
    # by hand: MOVE_NONE, a pass, a point off the board, an unplayable point, an empty row
    codes, mv = hand_rows()
    s = M.sums_host(codes, mv, *strengths(np.random.default_rng(4)))
    assert s.rank[[2, 3, 4, 5]].tolist() == [-1] * 4 and s.rank[0] == 40 and s.rank[1] == 0 and s.total[2] == 0
    assert M.sums_host(codes[:1], np.array([81]), *strengths(np.random.default_rng(4))).rank.tolist() == [-1]
    quiet = M.sums_host(codes[2:6], mv[2:6], *strengths(np.random.default_rng(4)))
    assert not quiet.den_p.any() and not quiet.den_t.any()


# ---- 5. the interface ----------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    a = M.parse_args(["fit", "-p", "w.bkw", "--patterns-out", "p.npy", "--tactics-out", "t.npy"])
    assert (a.games, a.seed, a.records, a.iterations, a.prior, a.scale) == (4096, 0, None, 20, 1.0, 64)
    a = M.parse_args(["fit", "--games", "0", "--records", "a", "b", "--iterations", "5", "--prior", "0.5", "--scale", "128",
                      "--patterns-out", "p.npy", "--tactics-out", "t.npy"])
    assert (a.p, a.games, a.records, a.iterations, a.prior, a.scale) == (None, 0, ["a", "b"], 5, 0.5, 128)
    a = M.parse_args(["eval", "--patterns", "p.npy", "--tactics", "t.npy", "-p", "w.bkw", "--games", "8", "--seed", "3"])
    assert (a.command, a.patterns, a.tactics, a.games, a.seed) == ("eval", "p.npy", "t.npy", 8, 3)
    out = ["--patterns-out", "p.npy", "--tactics-out", "t.npy"]
    for bad in (["fit", "-p", "w"], ["fit", "-p", "w", "--games", "0"] + out, ["fit", "--games", "4"] + out,
                ["fit", "-p", "w", "--games", "-1"] + out, ["fit", "-p", "w", "--iterations", "0"] + out,
                ["fit", "-p", "w", "--prior", "0"] + out, ["fit", "-p", "w", "--scale", "65536"] + out,
                ["fit", "-p", "w", "--seed", "-1"] + out, ["eval", "--games", "8"], ["eval", "-p", "w", "--games", "0"], []):
        with pytest.raises(SystemExit):
            M.parse_args(bad)
    capsys.readouterr()


def test_strengths_outside_the_domain_are_refused():
    codes, moves = hand_rows()
    gp, gt = strengths(np.random.default_rng(2))
    for name, entries, good in (("gp", PT.ENTRIES, gp), ("gt", TC.ENTRIES, gt)):
        assert T.mm_strengths(good, entries, name).dtype == torch.int32
        for value in (G_MIN - 1, G_MAX + 1, 0):
            bad = good.copy()
            bad[entries // 2] = value
            with pytest.raises(ValueError, match="strength"):
                T.mm_strengths(bad, entries, name)
            with pytest.raises(ValueError, match="strength"):
                M.sums_host(codes, moves, *((bad, gt) if name == "gp" else (gp, bad)))
        with pytest.raises(ValueError):
            T.mm_strengths(good[:-1], entries, name)
        with pytest.raises(ValueError):
            T.mm_strengths(good.astype(np.float64), entries, name)
    with pytest.raises(ValueError):
        M.step_tactics(np.full(TC.ENTRIES, G_MIN - 1), np.zeros(TC.ENTRIES, np.int64), np.zeros(TC.ENTRIES, np.uint64))
    # a step: the closed form, the clip, and an unseen feature half way to 1
    g = M.step_tactics(np.array([ONE, 4 * ONE, ONE, ONE] + [ONE] * 60), np.array([3, 0, 10 ** 9, 0] + [0] * 60),
                       np.array([2 << 32, 0, 0, 10 ** 9 << 32] + [0] * 60, np.uint64), prior=1.0)
    assert g[:4].tolist() == [round(ONE * 4 / 3), round(ONE * 2.5), G_MAX, G_MIN] and (g[4:] == ONE).all()


def test_header_binding_and_library_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_mm_sums\s*\(\s*const\s+uint32_t\s*\*\s*codes\s*,\s*const\s+int32_t\s*\*\s*moves\s*,\s*int\s+rows\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*gp\s*,\s*const\s+uint32_t\s*\*\s*gt\s*,\s*uint64_t\s*\*\s*den_p\s*,"
                     r"\s*uint64_t\s*\*\s*den_t\s*,\s*uint64_t\s*\*\s*total\s*,\s*uint64_t\s*\*\s*chosen\s*,"
                     r"\s*int32_t\s*\*\s*rank\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"#define\s+BKT_MM_MAX_ROWS\s+16384\b", src) and T.MM_MAX_ROWS == M.MAX_ROWS == 16384
    assert (T.MM_G_MIN, T.MM_G_MAX) == (1 << 8, 1 << 24)
    res, args = T.SYMBOLS["bkt_mm_sums"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, P, I, P, P, P, P, P, P, P, P] and callable(T.mm_sums)
    assert all(hasattr(M, name) for name in M.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_mm_sums
    make = open(os.path.join(CSRC, "Makefile")).read()
    (line,) = [l for l in make.splitlines() if l.startswith("\t") and "-o $@" in l and "bk_playout_pat.hip" in l]
    assert "bk_playout_mm.hip" in line.split()
    for name in ("bk_playout.hip", "bk_playout_mc.hip", "bk_playout_pat.hip", "bk_playout_tac.hip"):
        assert "bk_playout_mm" not in open(os.path.join(CSRC, name)).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_builds_alone_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_mm.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    assert len(blocks) == 1 and "mm_sums_kernel" in blocks[0].split()[0], [b.split()[0] for b in blocks]
    field = lambda pat: int(re.search(pat + r": (\d+)", blocks[0]).group(1))  # noqa: E731
    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field(r"SGPRs Spill") == 0 and field(r"VGPRs Spill") == 0, blocks[0]
    # 512 stone-free indices and 64 codes as uint64, the tactics strengths, and the waves' partial sums
    assert field(r"LDS Size \[bytes/block\]") == 512 * 8 + 64 * 8 + 64 * 4 + 4 * 2 * 8 + 3 * 8 + 4 * 2 * 4, blocks[0]
    assert field(r" VGPRs") <= 64 and field(r"Occupancy \[waves/SIMD\]") == 8, blocks[0]

"""Rows that put bkt_sample_moves at its float edges, with what the contract of include/bokego_train.h expects of them.
Shared by test_reinforce_cpu.py (the float64 mirror, lockstep.sample_host) and test_gpu_reinforce.py (the kernel), so
that both are held to the same rows and to expectations that come from neither of them.

A  indicator rows (logits in {0, -inf}): p is exactly 0 or 1 and every prefix an exact integer, so the move is known
   exactly for every draw, with no row excused.
B  rows whose sample is one illegal point whatever u is: the replacement rule and its tie-breaks.
C  x = s * z for spreads s from 0 to 200 (expf underflows from s = 40 on).
D  degenerate rows (a NaN, a +inf, all -inf) and their ordinary neighbours.
"""
import numpy as np

from bokego_amd import reinforce as R

SEED = 0xC0FFEE12345678
NEG = -np.inf


def draws(n, seed=SEED, ply=0):
    """counters int32 [n,4] as the existing sampler tests build them, and the first Philox word x0 uint32 [n] of each."""
    c = R.counters(np.arange(n), ply, 5, 9)
    return c, R.philox4x32_10(c.view(np.uint32), R.seed_key(seed))[:, 0]


def contract(x, legal):
    """What the contract gives without a draw, row by row in plain Python: (the replacement move, the row is degenerate).
    The replacement is the legal point of the largest logit, NaN ordered as -inf, lowest index on ties; -1 with none."""
    moves, deg = [], []
    for row, ok in zip(np.asarray(x), np.asarray(legal, bool)):
        deg.append(bool(np.isnan(row).any() or (row == np.inf).any() or (row == NEG).all()))
        best, at = None, -1
        for i in range(81):
            v = NEG if np.isnan(row[i]) else row[i]
            if ok[i] and (best is None or v > best):
                best, at = v, i
        moves.append(at)
    return np.array(moves, np.int32), np.array(deg)


# ---- A: indicator rows -------------------------------------------------------------------------------------------------
DRAWS_A = 4096


def indicator_supports():
    """The supports s_0 < ... < s_{n-1}: the edges of the register split (point 63 | point 64), the ends, whole halves,
    a stride, and 64 seeded random subsets."""
    fixed = [[80], [0], [63], [64], [63, 64], [0, 80], range(64), range(64, 81), range(81), range(0, 81, 3)]
    rng = np.random.default_rng(20261020)
    rand = [np.sort(rng.choice(81, size=int(rng.integers(1, 82)), replace=False)) for _ in range(64)]
    return [np.array(list(s), np.int64) for s in fixed] + rand


def indicator_rows():
    """-> (logits f32 [S,81], the supports, row_support int64 [S * DRAWS_A]): row r of the test has logits[row_support[r]]."""
    sup = indicator_supports()
    x = np.full((len(sup), 81), NEG, np.float32)
    for i, s in enumerate(sup):
        x[i, s] = 0.0
    return x, sup, np.repeat(np.arange(len(sup)), DRAWS_A)


def indicator_moves(sup, row_support, x0):
    """The exact move of every row: thr = fl32(fl32(k * 2^-24) * n) with k = x0 >> 8 (k * 2^-24 and n are exact in
    float32, so the product is the kernel's one rounding), and the first prefix above thr is that of s_j, j = floor(thr)."""
    n = np.array([len(s) for s in sup], np.float32)[row_support]
    thr = ((x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)) * n
    assert thr.dtype == np.float32
    j = np.floor(thr).astype(np.int64)
    assert (j < n).all()                                         # u * n rounds below n: (1 - 2^-24) * n is not n in float32
    flat = np.concatenate(sup)
    first = np.concatenate([[0], np.cumsum([len(s) for s in sup])])[:-1]
    return flat[first[row_support] + j].astype(np.int32), -np.log(n.astype(np.float64))


# ---- B: the replacement rule -------------------------------------------------------------------------------------------
DRAWS_B = 8
# (name, {legal point: logit}, the move).  The best legal logit is 4; every other point gets a seeded integer in -4..4, so
# illegal points hold 4s too, and lower indices than the answer: only the legal ones may count.
REPLACEMENT = [
    ("tie inside lane 5: points 5 and 69", {5: 4, 69: 4, 20: 3, 75: 2}, 5),
    ("tie inside lane 16: points 16 and 80", {16: 4, 80: 4, 50: 1}, 16),
    ("tie across lanes 12 and 47", {12: 3, 47: 3, 66: 1}, 12),
    ("tie of point 30 with point 70 of the lower lane 6", {30: 4, 70: 4, 2: 0}, 30),
    ("tie of points 66 and 72, both in the upper registers", {66: 2, 72: 2, 1: -3}, 66),
    ("tie of points 31 and 32 across the first exchange", {31: 1, 32: 1}, 31),
    ("best only at 80, its lane's point 16 legal and lower", {80: 4, 16: 1, 3: 0, 40: 3}, 80),
    ("best only at 64, its lane's point 0 legal and lower", {64: 4, 0: 2, 33: 3}, 64),
    ("best only at 63", {63: 4, 0: 3, 79: 3, 62: -4}, 63),
    ("single legal point 41", {41: -4}, 41),
    ("single legal point 77", {77: -4}, 77),
]
SAMPLED = (10, 71)        # the illegal point that is sampled, below and above the register split


def replacement_rows():
    """-> (logits f32 [n,81], legal bool [n,81], the moves int32 [n], names): each case with s = 10 and s = 70, DRAWS_B
    rows each.  x[s] = 60 against values <= 4: the prefix before s is below 81 * e^-56 < 2^-24 <= u * S whenever k > 0, and
    the prefix at s is >= 1 > u * S, so the sample is s for every draw with k > 0."""
    rng = np.random.default_rng(7)
    xs, ls, want, names = [], [], [], []
    for name, pts, mv in REPLACEMENT:
        for s in SAMPLED:
            assert s not in pts
            x = rng.integers(-4, 5, 81).astype(np.float32)
            legal = np.zeros(81, bool)
            for p, v in pts.items():
                x[p], legal[p] = v, True
            x[s] = 60.0
            xs += [x] * DRAWS_B
            ls += [legal] * DRAWS_B
            want += [mv] * DRAWS_B
            names += [f"{name}, s = {s}"] * DRAWS_B
    return np.stack(xs), np.stack(ls), np.array(want, np.int32), names


# ---- C: spreads ----------------------------------------------------------------------------------------------------------
SPREADS = (0, 0.01, 1, 10, 40, 200)
ROWS_C = 40000
_Z = []


def spread_rows(s):
    """x = s * z, float32 [ROWS_C, 81]; z is drawn once and shared by every spread."""
    if not _Z:
        _Z.append(np.random.default_rng(20261020).standard_normal((ROWS_C, 81), dtype=np.float32))
    return np.float32(s) * _Z[0]


# ---- D: degenerate rows ----------------------------------------------------------------------------------------------------
DRAWS_D = 4
LEGAL_SETS = {"point 0 legal": (0, 7, 40, 64, 80), "point 0 illegal": (7, 40, 64, 80), "no legal point": ()}


def _f32_bits(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def degenerate_rows():
    """-> (logits f32 [n,81], legal bool [n,81], names): every kind of row below with each of LEGAL_SETS, DRAWS_D rows
    (draws) each.  The finite values are seeded normals, largest at the illegal point 23."""
    base = np.random.default_rng(11).standard_normal(81).astype(np.float32)
    base[23] = 5.0
    xs, ls, names = [], [], []
    for lname, pts in LEGAL_SETS.items():
        legal = np.zeros(81, bool)
        legal[list(pts)] = True
        kinds = {}
        kinds["all NaN"] = np.full(81, np.nan, np.float32)
        kinds["one NaN at the legal point 40"] = base.copy()
        kinds["one NaN at the legal point 40"][40] = np.nan
        kinds["one NaN at the illegal point 23"] = base.copy()
        kinds["one NaN at the illegal point 23"][23] = np.nan
        kinds["a negative and a signalling NaN"] = base.copy()
        kinds["a negative and a signalling NaN"][[12, 70]] = _f32_bits(0xFFC00001), _f32_bits(0x7F800001)
        kinds["+inf at the legal point 64"] = base.copy()
        kinds["+inf at the legal point 64"][64] = np.inf
        kinds["+inf at the illegal point 70"] = base.copy()
        kinds["+inf at the illegal point 70"][70] = np.inf
        kinds["all -inf"] = np.full(81, NEG, np.float32)
        kinds["NaN at exactly the legal points"] = base.copy()
        kinds["NaN at exactly the legal points"][legal] = np.nan          # with no legal point: an ordinary finite row
        kinds["legal logits all -inf among finite illegal ones"] = base.copy()
        kinds["legal logits all -inf among finite illegal ones"][legal] = NEG   # ordinary: the draw lands outside the set
        for kname, x in kinds.items():
            xs += [x] * DRAWS_D
            ls += [legal] * DRAWS_D
            names += [f"{kname}; {lname}"] * DRAWS_D
    return np.stack(xs), np.stack(ls), names

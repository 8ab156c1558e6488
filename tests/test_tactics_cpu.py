"""CPU: the tactical playouts that need no GPU -- the tactical code by hand and against a second formulation,
the combined weight at its extremes, neutral tables against the pattern and the uniform host games, the fit (counts,
weights), the table file, the callers and command lines, the declarations and the bindings, and the kernels' resources when
compiled for gfx950."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match
from bokego_amd import lockstep as L
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import REPO
from test_playout_value_cpu import _FakeEngine, golden_records
from test_rollout_cpu import BOARD, records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"


def planes_of(recs):
    F = np.empty((len(recs), 27, 81), np.uint8)
    L.features_batch(np.array(recs, np.uint8, order="C"), F.ctypes.data)
    return F


def slow_codes(recs):
    """The definition, point by point, in plain Python on the planes."""
    F = planes_of(recs)
    out = np.zeros((len(recs), 81), np.int32)
    for i in range(len(recs)):
        for q in range(81):
            cap = max(int(v) for v in F[i, 20:27, q])
            la = max(int(v) for v in F[i, 13:20, q])
            r, c = divmod(q, 9)
            nbrs = [9 * rr + cc for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)) if 0 <= rr < 9 and 0 <= cc < 9]
            e = any(F[i, 0, t] and F[i, 6, t] for t in nbrs)
            g = any(F[i, 1, t] and F[i, 7, t] for t in nbrs)
            out[i, q] = min(cap, 3) | (0 if la <= 1 else 1 if la == 2 else 2) << 2 | int(e) << 4 | int(g) << 5
    return out


@pytest.fixture(scope="module")
def goldens():
    return golden_records(536)


# ---- the code -------------------------------------------------------------------------------------------------------------------
def test_hand_checked_codes():
    board = "OX" + "." * 79                                             # white at point 0, black at point 1
    black = TC.codes_host(records([go.Game(board, turn=0)]))
    white = TC.codes_host(records([go.Game(board, turn=1)]))
    assert black.shape == (1, 81) and black.dtype == np.int32
    assert black[0, 9] == 9                                             # captures one stone; three liberties afterwards
    assert black[0, 2] == 8 and black[0, 40] == 8
    assert white[0, 9] == 20                                            # extends out of atari to two liberties
    assert white[0, 2] == 36                                            # gives atari; two liberties
    assert white[0, 40] == 8
    # occupied points have a code too: C = A = 0, and E, G from their neighbours (white's own stone at 0 has one liberty,
    # the black stone at 1 two)
    assert black[0, 0] == 0 and black[0, 1] == 0 and white[0, 1] == 1 << 4 and white[0, 0] == 1 << 5
    empty = TC.codes_host(records([go.Game()]))[0]
    corners = [0, 8, 72, 80]                                            # two liberties in a corner, three or four elsewhere
    assert (empty[corners] == 4).all() and (np.delete(empty, corners) == 8).all()
    assert TC.codes_host(np.zeros((0, 192), np.uint8)).shape == (0, 81)


def test_codes_against_a_second_formulation(goldens):
    assert len(goldens) == 536
    before = goldens.copy()
    codes = TC.codes_host(goldens)
    assert np.array_equal(goldens, before)                              # the records are not modified
    assert np.array_equal(codes, slow_codes(goldens))
    assert codes.min() >= 0 and codes.max() < TC.ENTRIES and not ((codes >> 2) & 3 == 3).any()
    legal = planes_of(goldens)[:, 5] != 0
    on = codes[legal]
    assert len(np.unique(on)) == 22
    for c in (1, 2, 3):
        assert ((on & 3) == c).any(), c
    assert ((on >> 4) & 1).any() and ((on >> 5) & 1).any() and (((on >> 2) & 3) == 0).any()
    # the census of the data the feature is exercised by
    cap, ext, atari = (codes & 3) > 0, ((codes >> 4) & 1) > 0, ((codes >> 5) & 1) > 0
    assert [(int((m & legal).sum()), int((m & legal).any(1).sum())) for m in (cap, ext, atari)] == [(69, 65), (116, 106),
                                                                                                   (783, 263)]
    # the other colour to move is another record with its own codes
    flipped = goldens[:50].copy()
    flipped[:, 172] ^= 1
    assert np.array_equal(TC.codes_host(flipped), slow_codes(flipped))
    assert all(isinstance(TC.describe(c), str) for c in range(TC.ENTRIES))


# ---- the draw -------------------------------------------------------------------------------------------------------------------
def test_combine_at_its_extremes_and_the_row_sum():
    assert TC.NEUTRAL == 256 and TC.ENTRIES == T.TACTIC_ENTRIES == 64
    w = TC.combine(np.array([65535, 65535, 0, 1, 300]), np.array([65535, 0, 256, 255, 256]))
    assert w.dtype == np.uint64
    assert w.tolist() == [65535 * 65535 >> 8, 1, 1, 1, 300]            # T = 0 -> 1; an entry of 0 is 1; 255 >> 8 = 0 -> 1
    assert int(w[0]) == 16776704 < 2 ** 24 and 65535 * 65535 < 2 ** 32  # the 32-bit product
    assert TC.combine(None, np.array([256, 0, 65535, 512])).tolist() == [256, 1, 65535, 512]     # no table: P = 256
    S = 81 * int(w[0])
    assert S < 2 ** 31 and (0xFFFFFFFF >> 8) * S < 2 ** 64
    # the full row: every point playable at the largest weight; both ends of the word are reached
    ok = np.ones((2, 81), bool)
    x0 = np.array([0, 0xFFFFFFFF], np.uint32)
    assert TC.select_tactical(x0, np.full((2, 81), 65535), np.full((2, 81), 65535), ok).tolist() == [0, 80]
    assert TC.select_tactical(x0, None, np.full((2, 81), 65535), np.zeros((2, 81), bool)).tolist() == [go.PASS, go.PASS]
    # against Python integers
    rng = np.random.default_rng(6)
    words = np.array([0, 1, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF, 0x12345678], np.uint32)
    P, Tt = rng.integers(0, 65536, (len(words), 81)), rng.integers(0, 65536, (len(words), 81))
    ok = rng.random((len(words), 81)) < 0.5
    for entries in (P, None):
        got = TC.select_tactical(words, entries, Tt, ok)
        for i, x in enumerate(words.tolist()):
            ws = [max(1, ((max(int(P[i, s]), 1) if entries is not None else 256) * int(Tt[i, s])) >> 8) if ok[i, s] else 0
                  for s in range(81)]
            t, acc = ((x >> 8) * sum(ws)) >> 24, 0
            for s in range(81):
                acc += ws[s]
                if acc > t:
                    break
            assert got[i] == s, (i, entries is None)


@pytest.fixture(scope="module")
def starts():
    """8 games from the empty board and 8 golden mid-game positions."""
    return np.concatenate([records([go.Game()] * 8), golden_records(8, 60)])


@pytest.fixture(scope="module")
def pattern_table():
    rng = np.random.default_rng(1)
    return PT.PatternTable(rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16))


def _same_games(a, b):
    return (np.array_equal(a.moves, b.moves) and np.array_equal(a.records, b.records) and np.array_equal(a.plies, b.plies)
            and np.array_equal(a.over, b.over) and np.array_equal(a.score, b.score) and np.array_equal(a.owner, b.owner))


def test_neutral_tactics_play_the_pattern_and_the_uniform_games(starts, pattern_table):
    neutral = TC.TacticTable.neutral()
    assert _same_games(RO.random_playouts(starts, 11, rules="host", patterns=pattern_table, tactics=neutral),
                       RO.random_playouts(starts, 11, rules="host", patterns=pattern_table))
    assert _same_games(RO.random_playouts(starts, 11, rules="host", tactics=neutral),
                       RO.random_playouts(starts, 11, rules="host"))


def test_a_table_changes_the_games_and_the_value_follows(starts, pattern_table):
    rng = np.random.default_rng(2)
    tactics = TC.TacticTable(rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16))
    before = starts.copy()
    plain = RO.random_playouts(starts, 11, rules="host", patterns=pattern_table)
    fin = RO.random_playouts(starts, 11, rules="host", patterns=pattern_table, tactics=tactics)
    assert np.array_equal(starts, before) and not np.array_equal(fin.moves[:, :20], plain.moves[:, :20])
    # replay a mid-game row by the definition
    g = 10
    rec = starts[g:g + 1].copy()
    ctr = RO.default_counters(len(starts), RO.record_turns(starts)).view(np.uint32)[g].copy()
    for k in range(int(fin.plies[g])):
        x0 = int(L.philox4x32_10(ctr[None], L.seed_key(11))[0, 0])
        pts = np.nonzero(RO.playable_host(rec)[0])[0]
        pc, tc = PT.codes_host(rec)[0], slow_codes(rec)[0]
        ws = [max(1, (max(int(pattern_table.array[pc[s]]), 1) * int(tactics.array[tc[s]])) >> 8) for s in pts]
        t, acc, want = ((x0 >> 8) * sum(ws)) >> 24, 0, go.PASS
        for s, w in zip(pts.tolist(), ws):
            acc += w
            if acc > t:
                want = s
                break
        assert fin.moves[g, k] == want, k
        L.play_host(rec, [0], [want], lambda r, m: f"illegal {m}", liberties=True)
        ctr[1] += np.uint32(1)
    assert np.array_equal(rec[0], fin.records[g])
    # playout_value: a pure function of the record, through both tables
    recs = starts[6:12]
    v = RO.playout_value(recs, 4, 3, rules="host", patterns=pattern_table, tactics=tactics)
    assert np.array_equal(RO.playout_value(recs[::-1], 4, 3, rules="host", patterns=pattern_table, tactics=tactics), v[::-1])
    assert np.array_equal(RO.playout_value(recs, 4, 3, rules="host", tactics=TC.TacticTable.neutral()),
                          RO.playout_value(recs, 4, 3, rules="host"))
    many = golden_records(24, 20)
    assert not np.array_equal(RO.playout_value(many, 4, 3, rules="host", tactics=tactics),
                              RO.playout_value(many, 4, 3, rules="host"))
    # the board that needs no luck plays its one game under any table
    fin = RO.random_playouts(records([go.Game(BOARD)] * 2), 3, rules="host", tactics=tactics)
    assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 2 and fin.score.tolist() == [3.5] * 2
    with pytest.raises(ValueError, match="one_launch"):
        RO.rollout_score([go.Game(BOARD)], None, n=2, rules="host", tactics=tactics)
    r = RO.rollout_score([go.Game(BOARD)], None, n=2, rules="host", one_launch=True, tactics=tactics)[0]
    assert r.score == 3.5


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def test_weights_exact_values_and_clipping():
    mass = np.array([0.0, 16.0, 48.0, 0.0, 1e9, 0.0, 100.0, 3.5])
    played = np.array([0, 16, 0, 16, 0, 10 ** 6, 50, 7], np.int64)
    w = TC.weights(mass, played)
    assert w.dtype == np.uint16
    # floor(256 * (played + 16) / (mass + 16) + 1/2): neutral, neutral, 256 / 4 = 64, 512, ~0 -> clipped to 1,
    # 256 * 1000016 / 16 -> clipped to 65535, 256 * 66 / 116 = 145.66, 256 * 23 / 19.5 = 301.95
    assert w.tolist() == [256, 256, 64, 512, 1, 65535, 146, 302]
    assert TC.weights([1.0], [0], prior=1.0).tolist() == [128] and TC.weights([0.0], [1], prior=1.0).tolist() == [512]
    assert TC.weights([511.0], [0], prior=1.0).tolist() == [1]          # 0.5 rounds up
    assert TC.weights([1023.0], [0], prior=1.0).tolist() == [1]         # 0.25 rounds to 0: clipped to 1
    for bad in (0, -1.0):
        with pytest.raises(ValueError):
            TC.weights(mass, played, prior=bad)


def test_counts_of_a_hand_made_game_with_a_capture(pattern_table):
    # black 1, white 0 (the corner), black 9 captures it, white 40
    moves = np.array([[1, 0, 9, 40, RO.MOVE_NONE]], np.int16)
    start = records([go.Game()])
    mass, played = TC.counts(start, moves, rules="host")
    assert mass.dtype == np.float64 and played.dtype == np.int64 and mass.shape == played.shape == (TC.ENTRIES,)
    assert played.sum() == 4 and abs(mass.sum() - 4.0) < 1e-12          # one expected play per ply
    assert played[8] == 2 and played[0] == 1 and played[9] == 1         # 1 and 40: 3+ liberties; the corner: 1 liberty; the capture
    # ply 2 is the "OX" board with black to move: 79 playable points, the capture (code 9) among them
    assert abs(mass[9] - 1 / 79) < 1e-15
    # the whole histogram against a recount by the definition
    want_mass, want_played = np.zeros(TC.ENTRIES), np.zeros(TC.ENTRIES, np.int64)
    for table, (got_mass, got_played) in ((None, (mass, played)),
                                          (pattern_table, TC.counts(start, moves, pattern_table, rules="host"))):
        want_mass[:], want_played[:] = 0, 0
        g = go.Game()
        for mv in moves[0, :4].tolist():
            rec = records([g])
            pts = np.nonzero(RO.playable_host(rec)[0])[0].tolist()
            tc, pc = slow_codes(rec)[0], PT.codes_host(rec)[0]
            P = [1.0 if table is None else float(max(int(table.array[pc[s]]), 1)) for s in pts]
            for s, p in zip(pts, P):
                want_mass[tc[s]] += p / sum(P)
            want_played[tc[mv]] += 1
            g.play_move(mv)
        assert np.array_equal(got_played, want_played) and np.allclose(got_mass, want_mass, rtol=1e-12, atol=0)
    assert np.array_equal(TC.counts(start, moves, pattern_table, rules="host")[1], played)    # the moves are the moves
    table = TC.fit(start, moves, rules="host", prior=1.0)
    assert isinstance(table, TC.TacticTable) and np.array_equal(table.array, TC.weights(mass, played, prior=1.0))
    assert table.array[9] > 256 and table.array[63] == 256             # the capture was taken; an unseen code stays neutral
    # a move into the mover's own eye adds to mass only; an illegal move raises
    mass, played = TC.counts(records([go.Game(BOARD)]), np.array([[0]], np.int16), rules="host")
    assert abs(mass.sum() - 1.0) < 1e-12 and played.sum() == 0
    with pytest.raises(RuntimeError, match="illegal"):
        TC.counts(records([go.Game(BOARD)]), np.array([[1]], np.int16), rules="host")
    with pytest.raises(ValueError):
        TC.counts(start, np.array([40], np.int16), rules="host")


def test_the_table_file(tmp_path):
    rng = np.random.default_rng(3)
    table = TC.TacticTable(rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16))
    path = str(tmp_path / "tactics.npy")
    table.save(path)
    assert np.array_equal(TC.TacticTable.load(path).array, table.array)
    assert np.array_equal(np.load(path), table.array)                   # a plain .npy
    assert np.array_equal(TC.as_tactics(path).array, table.array) and TC.as_tactics(table) is table
    assert TC.as_tactics(None) is None and np.array_equal(TC.as_tactics(table.array).array, table.array)
    assert (TC.TacticTable.neutral().array == 256).all() and TC.TacticTable.neutral().array.shape == (64,)
    for bad in (np.zeros(64, np.int16), np.zeros(64, np.float32), np.zeros(63, np.uint16), np.zeros((2, 32), np.uint16),
                np.zeros(PT.ENTRIES, np.uint16)):
        with pytest.raises(ValueError, match="tactics table"):
            TC.TacticTable(bad)
        np.save(str(tmp_path / "bad.npy"), bad)
        with pytest.raises(ValueError, match="tactics table"):
            TC.TacticTable.load(str(tmp_path / "bad.npy"))
    assert TC.show(TC.TacticTable.neutral()) == "every entry is neutral"
    text = TC.show(table)
    assert text.count("code") == (table.array[[c for c in range(64) if (c >> 2) & 3 != 3]] != 256).sum()
    assert TC.describe(9) == "captures 1, 3+ liberties after" and "atari" in TC.describe(20)


# ---- the callers ----------------------------------------------------------------------------------------------------------------
def test_native_mcts_takes_the_table(tmp_path, pattern_table):
    class Net:
        def engine(self):
            return _FakeEngine()

    rng = np.random.default_rng(4)
    table = TC.TacticTable(rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16))
    path = str(tmp_path / "t.npy")
    table.save(path)
    policy = lambda x: np.zeros((len(x), 81), np.float32)            # noqa: E731
    with pytest.raises(TypeError, match="playout_tactics"):
        NativeMCTS(Position(), policy, policy, playout_tactics=table)
    for given in (table, path):
        t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_tactics=given, playout_rules="host",
                       expand_thresh=1)
        assert isinstance(t.evaluator.tactics, TC.TacticTable) and np.array_equal(t.evaluator.tactics.array, table.array)
        assert t.evaluator.patterns is None
        t.rollout(6)
        assert t.root.value == 1.0 and t.choose().last_move == 38
        t.close()
    t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_patterns=pattern_table, playout_tactics=table,
                   playout_rules="host")
    assert t.evaluator.patterns is pattern_table and t.evaluator.tactics is table
    t.close()
    t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_rules="host")
    assert t.evaluator.tactics is None
    t.close()
    ev = RO.PlayoutEvaluator(_FakeEngine(), 3, seed=4, rules="host", patterns=pattern_table, tactics=table)
    recs = golden_records(4, 90)
    assert np.array_equal(ev(recs, 0)[1], RO.playout_value(recs, 3, 4, rules="host", patterns=pattern_table, tactics=table))


def test_command_lines(capsys):
    a = TC.parse_args(["fit", "-p", "w.bkw", "--games", "64", "--seed", "3", "--patterns", "p.npy", "-o", "t.npy"])
    assert (a.command, a.p, a.games, a.seed, a.patterns, a.o, a.prior) == ("fit", "w.bkw", 64, 3, "p.npy", "t.npy", 16.0)
    a = TC.parse_args(["fit", "-p", "w.bkw", "-o", "t.npy"])
    assert a.games == 4096 and a.patterns is None
    a = TC.parse_args(["show", "t.npy"])
    assert (a.command, a.table) == ("show", "t.npy")
    for bad in (["fit", "-o", "t.npy"], ["fit", "-p", "w"], ["fit", "-p", "w", "-o", "t", "--games", "0"],
                ["fit", "-p", "w", "-o", "t", "--seed", "-1"], ["fit", "-p", "w", "-o", "t", "--prior", "0"], ["show"], []):
        with pytest.raises(SystemExit):
            TC.parse_args(bad)
    assert gtp.parse_args([]).playout_tactics is None and match.parse_args([]).playout_tactics is None
    a = gtp.parse_args(["--playout-value", "64", "--playout-tactics", "t.npy"])
    assert a.playout_value == 64 and a.playout_tactics == "t.npy" and a.playout_patterns is None
    a = match.parse_args(["--playout-value", "64", "--playout-patterns", "p.npy", "--playout-tactics", "t.npy"])
    assert a.playout_value == 64 and a.playout_tactics == "t.npy" and a.playout_patterns == "p.npy"
    for bad in (["--playout-tactics", "t.npy"], ["--playout-tactics", "t.npy", "--playout-value", "0"],
                ["--playout-value", "8", "--playout-tactics", "t.npy", "-v", "v.pt"],
                ["--playout-value", "8", "--playout-tactics", "t.npy", "--simulate"],
                ["--playout-value", "8", "--playout-tactics", "t.npy", "--python-tree"]):
        with pytest.raises(SystemExit):
            gtp.parse_args(bad)
    for bad in (["--playout-tactics", "t.npy"],
                ["--playout-value", "8", "--playout-tactics", "t.npy", "--engine", "python -m oracle.gtp_cpu"]):
        with pytest.raises(SystemExit):
            match.parse_args(bad)
    a = RO._parse(["--sgf", "g.sgf", "--random", "--tactics", "t.npy"])
    assert a.random and a.tactics == "t.npy" and a.patterns is None and RO._parse(["--sgf", "g.sgf", "--random"]).tactics is None
    with pytest.raises(SystemExit):
        RO._parse(["--sgf", "g.sgf", "--tactics", "t.npy"])
    capsys.readouterr()


# ---- the declarations, the bindings, the build ------------------------------------------------------------------------------
def test_header_and_binding():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_TACTIC_ENTRIES\s+64\b", src) and T.TACTIC_ENTRIES == TC.ENTRIES == 64
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_tactical_codes\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*int32_t\s*\*\s*codes\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+bkt_tactical_playouts\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*int\s+max_plies\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,"
                     r"\s*int32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", code)
    res, args = T.SYMBOLS["bkt_tactical_playouts"]
    assert res is ctypes.c_int and len(args) == 12 and args[2] is ctypes.c_uint64 and args[1] is args[6] is ctypes.c_int
    same = T.SYMBOLS["bkt_pattern_playouts"][1]
    assert args[:5] == same[:5] and args[6:] == same[5:] and args[5] is ctypes.c_void_p       # tactics put in after table
    res, args = T.SYMBOLS["bkt_tactical_codes"]
    assert (res, args) == T.SYMBOLS["bkt_pattern_codes"]
    assert callable(T.tactical_playouts) and callable(T.tactical_codes)
    assert all(hasattr(TC, name) for name in TC.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_tactical_playouts and lib.bkt_tactical_codes
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"-shared bk_train\.hip bk_train_bf16\.hip bk_playout_pat\.hip -o", make)
    assert re.search(r"^\$\(TRAIN_OUT\):.*\bbk_playout_tac\.hip\b", make, flags=re.M)          # a dependency, not a source
    assert '#include "bk_playout_tac.hip"' in open(os.path.join(CSRC, "bk_playout_pat.hip")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernels_build_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    for name in ("tactical_playouts_kernel", "tactical_codes_kernel"):
        mine = [b for b in blocks if name in b.split()[0]]
        assert len(mine) == 1, [b.split()[0] for b in blocks]
        spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", mine[0])
        scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0])
        assert len(spills) == 2 and len(scratch) == 1
        assert all(int(n) == 0 for _, n in spills), (name, spills)
        assert int(scratch[0]) == 0, (name, scratch)

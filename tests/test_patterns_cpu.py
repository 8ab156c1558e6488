"""CPU: the pattern-weighted playouts that need no GPU -- the 3x3 pattern index by hand and under the eight
symmetries, the weighted integer draw against Python integers, constant tables against the uniform host games, the fit
(counts, symmetrise, weights), the table file, the command lines, the declarations and the bindings, and the kernels'
resources when compiled for gfx950."""
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
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import REPO
from test_playout_value_cpu import _FakeEngine, golden_records
from test_rollout_cpu import BOARD, records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
NEAR = 1 << 16


def slow_index(rec, s):
    """The definition, point by point, in plain Python."""
    board, turn = rec[:81], int(rec[172:176].view(np.int32)[0])
    lm = int(rec[166:168].view(np.int16)[0])
    me = 2 if turn & 1 else 1
    r, c = divmod(s, 9)
    code = 0
    for i, (dr, dc) in enumerate([(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]):
        rr, cc = r + dr, c + dc
        if not (0 <= rr < 9 and 0 <= cc < 9):
            st = 3
        else:
            st = 0 if board[9 * rr + cc] == 0 else 1 if board[9 * rr + cc] == me else 2
        code |= st << (2 * i)
    near = 0 <= lm < 81 and max(abs(r - lm // 9), abs(c - lm % 9)) <= 1
    return (NEAR if near else 0) | code


def set_header(rec, turn=None, last_move=None):
    rec = rec.copy()
    if turn is not None:
        rec[172:176] = np.array([turn], np.int32).view(np.uint8)
    if last_move is not None:
        rec[166:168] = np.array([last_move], np.int16).view(np.uint8)
    return rec


# ---- the index ------------------------------------------------------------------------------------------------------------------
def test_hand_computed_indices():
    empty = records([go.Game()])
    codes = PT.codes_host(empty)
    assert codes.shape == (1, 81) and codes.dtype == np.int32
    assert codes[0, 0] == 3 | 3 << 4 | 3 << 8 | 3 << 10 | 3 << 12        # slots 0, 2, 4, 5, 6 are off the board
    assert codes[0, 40] == 0 and (codes[0] < NEAR).all()                   # no last move: near nowhere
    assert codes[0, 80] == 3 << 2 | 3 << 6 | 3 << 10 | 3 << 12 | 3 << 14  # slots 1, 3, 5, 6, 7
    assert codes[0, 4] == 3 | 3 << 8 | 3 << 10 and codes[0, 36] == 3 << 4 | 3 << 8 | 3 << 12
    # a black stone north of s = 40: state 1 in slot 0 with black to move, 2 with white to move
    g = go.Game()
    g.play_move(31)
    rec = records([g])[0]
    assert not L.black_to_move(rec[None])[0]
    assert PT.codes_host(rec[None])[0, 40] == (NEAR | 2)
    assert PT.codes_host(set_header(rec, turn=2)[None])[0, 40] == (NEAR | 1)
    # near: exactly the up-to-9 points around a last move; none after a pass or without a move
    for lm, want in ((31, 9), (0, 4), (8, 4), (4, 6), (45, 6), (80, 4)):
        near = PT.codes_host(set_header(rec, last_move=lm)[None])[0] >= NEAR
        pts = [s for s in range(81) if max(abs(s // 9 - lm // 9), abs(s % 9 - lm % 9)) <= 1]
        assert np.nonzero(near)[0].tolist() == pts and len(pts) == want, lm
    for lm in (go.PASS, -3):
        assert (PT.codes_host(set_header(rec, last_move=lm)[None]) < NEAR).all()
    after = go.Game()
    after.play_move(31)
    after.play_pass()
    assert (PT.codes_host(records([after])) < NEAR).all()
    # every point of some real positions against the definition
    recs = golden_records(6, 70)
    codes = PT.codes_host(recs)
    assert all(codes[i, s] == slow_index(recs[i], s) for i in range(len(recs)) for s in range(81))
    assert codes.max() < PT.ENTRIES and codes.min() >= 0


def test_the_eight_symmetries():
    perms = [PT.slot_permutation(g) for g in range(8)]
    assert perms[0] == list(range(8)) and len({tuple(p) for p in perms}) == 8
    assert all(sorted(p) == list(range(8)) and sorted(p[:4]) == [0, 1, 2, 3] for p in perms)    # sides stay sides
    pts = np.arange(81)
    recs = golden_records(5, 90)
    base = PT.codes_host(recs)
    for g in range(8):
        to = PT.transform_point(pts, g)
        assert sorted(to.tolist()) == list(range(81)) and to[40] == 40
        assert PT.transform_point(np.array([go.PASS, -3]), g).tolist() == [go.PASS, -3]
        moved = recs.copy()
        moved[:, to] = recs[:, :81]
        lm = L.record_last_move(recs).astype(np.int64)
        moved[:, 166:168] = PT.transform_point(lm, g).astype(np.int16)[:, None].view(np.uint8)
        got = PT.codes_host(moved)
        assert np.array_equal(got[:, to], PT.transform_code(base, g)), g
    # near is invariant, and a transformed code is a code
    idx = np.arange(PT.ENTRIES)
    for g in range(8):
        t = PT.transform_code(idx, g)
        assert np.array_equal(t & NEAR, idx & NEAR) and sorted(t.tolist()) == idx.tolist()


# ---- the draw -------------------------------------------------------------------------------------------------------------------
WORDS = [0, 1, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF, 0x12345678]


def slow_pick(x0, w):
    w = [max(int(v), 1) for v in w]
    t = ((x0 >> 8) * sum(w)) >> 24
    acc = 0
    for i, v in enumerate(w):
        acc += v
        if acc > t:
            return i
    raise AssertionError("t >= S")


def test_the_weighted_draw():
    assert 81 * 65535 < 2 ** 23 and (0xFFFFFFFF >> 8) * 81 * 65535 < 2 ** 47
    rng = np.random.default_rng(5)
    rows = [np.full(81, 65535), np.full(81, 1), np.array([65535]), np.array([0]), np.array([0, 0, 7]),
            rng.integers(0, 65536, 81), rng.integers(0, 65536, 33), rng.integers(0, 3, 50)]
    for w in rows:
        for x0 in WORDS:
            assert PT.weighted_pick(x0, w) == slow_pick(x0, w), (x0, w[:4])
        assert PT.weighted_pick(0, w) == 0 and PT.weighted_pick(0xFFFFFFFF, w) == len(w) - 1    # both ends are reached
    # the largest S: the product does not wrap in uint64, and in 32 bits it would
    assert (0xFFFFFFFF >> 8) * 81 * 65535 >= 2 ** 32
    # rows: entries of every point, weights only where playable; an empty row passes
    entries = rng.integers(0, 65536, (len(WORDS), 81))
    ok = rng.random((len(WORDS), 81)) < 0.4
    ok[3] = False
    got = PT.select_weighted(np.array(WORDS, np.uint32), entries, ok)
    for i, x0 in enumerate(WORDS):
        pts = np.nonzero(ok[i])[0]
        assert got[i] == (go.PASS if len(pts) == 0 else pts[slow_pick(x0, entries[i, pts])]), i
    # an entry of 0 behaves as 1
    zero = np.where(entries == 0, 1, entries)
    assert np.array_equal(PT.select_weighted(np.array(WORDS, np.uint32), np.zeros_like(entries), ok),
                          PT.select_weighted(np.array(WORDS, np.uint32), np.ones_like(entries), ok))
    assert np.array_equal(PT.select_weighted(np.array(WORDS, np.uint32), zero, ok), got)
    with pytest.raises(ValueError):
        PT.weighted_pick(5, np.array([]))
    # a constant weight selects the uniform rank, for every n and constant
    for n in (1, 2, 7, 80, 81):
        for c in (1, 7, 65535):
            for x0 in WORDS:
                assert PT.weighted_pick(x0, np.full(n, c)) == int(RO.select_index(x0, n)), (n, c, x0)


@pytest.fixture(scope="module")
def starts():
    """16 games from the empty board and 8 golden mid-game positions."""
    return np.concatenate([records([go.Game()] * 16), golden_records(8, 60)])


@pytest.fixture(scope="module")
def uniform(starts):
    return RO.random_playouts(starts, 11, rules="host")


@pytest.mark.parametrize("c", [1, 7, 65535, 0])
def test_a_constant_table_plays_the_uniform_games(starts, uniform, c):
    fin = RO.random_playouts(starts, 11, rules="host", patterns=PT.PatternTable.constant(c))
    assert np.array_equal(fin.moves, uniform.moves) and np.array_equal(fin.records, uniform.records)
    assert np.array_equal(fin.plies, uniform.plies) and np.array_equal(fin.over, uniform.over)
    assert np.array_equal(fin.score, uniform.score)


def test_a_table_changes_the_games_and_the_value_follows(starts, uniform):
    rng = np.random.default_rng(1)
    table = PT.PatternTable(rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16))
    before = starts.copy()
    fin = RO.random_playouts(starts, 11, rules="host", patterns=table)
    assert np.array_equal(starts, before) and not np.array_equal(fin.moves[:, :20], uniform.moves[:, :20])
    assert fin.over.sum() >= 20
    # replay game 0 and game 20 by the definition
    for g in (0, 20):
        rec = starts[g:g + 1].copy()
        ctr = RO.default_counters(len(starts), RO.record_turns(starts)).view(np.uint32)[g].copy()
        for k in range(int(fin.plies[g])):
            x0 = int(L.philox4x32_10(ctr[None], L.seed_key(11))[0, 0])
            pts = np.nonzero(RO.playable_host(rec)[0])[0]
            want = go.PASS if len(pts) == 0 else int(pts[slow_pick(x0, [table.array[slow_index(rec[0], s)] for s in pts])])
            assert fin.moves[g, k] == want, (g, k)
            L.play_host(rec, [0], [want], lambda r, m: f"illegal {m}", liberties=True)
            ctr[1] += np.uint32(1)
        assert np.array_equal(rec[0], fin.records[g])
    # playout_value: a pure function of the record, through the table
    recs = starts[14:20]
    v = RO.playout_value(recs, 4, 3, rules="host", patterns=table)
    assert np.array_equal(RO.playout_value(recs[::-1], 4, 3, rules="host", patterns=table), v[::-1])
    assert np.array_equal(RO.playout_value(recs, 4, 3, rules="host", patterns=PT.PatternTable.constant(9)),
                          RO.playout_value(recs, 4, 3, rules="host"))
    # the board that needs no luck plays its one game under any table
    fin = RO.random_playouts(records([go.Game(BOARD)] * 2), 3, rules="host", patterns=table)
    assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 2 and fin.score.tolist() == [3.5] * 2
    with pytest.raises(ValueError, match="one_launch"):
        RO.rollout_score([go.Game(BOARD)], None, n=2, rules="host", patterns=table)
    r = RO.rollout_score([go.Game(BOARD)], None, n=2, rules="host", one_launch=True, patterns=table)[0]
    assert r.score == 3.5


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def test_weights_exact_values_and_clipping():
    seen = np.array([0, 32, 96, 0, 10 ** 9, 0, 1000], np.int64)
    played = np.array([0, 32, 0, 31, 0, 10 ** 6, 500], np.int64)
    w = PT.weights(seen, played)
    assert w.dtype == np.uint16
    # round(1024 * (played + 1) / (seen + 32)): 32, 1024 * 33 / 64 = 528, 1024 / 128 = 8, 1024 * 32 / 32 = 1024,
    # ~0 -> clipped to 1, 1024 * 1000001 / 32 -> clipped to 65535, 1024 * 501 / 1032 = 497.1
    assert w.tolist() == [32, 528, 8, 1024, 1, 65535, 497]
    assert PT.weights([0], [0], scale=1, prior_seen=2).tolist() == [1]        # 1 * 1 / 2 = 0.5 rounds up
    assert PT.weights([1], [0], scale=1, prior_seen=2).tolist() == [1]        # 1/3 rounds to 0: clipped to 1
    assert PT.weights([0], [2], scale=100, prior_played=0, prior_seen=3).tolist() == [67]


def test_counts_of_a_hand_made_game():
    moves = np.array([[40, 0, go.PASS, 41, RO.MOVE_NONE]], np.int16)
    seen, played = PT.counts(records([go.Game()]), moves, rules="host")
    assert seen.dtype == played.dtype == np.int64 and seen.shape == played.shape == (PT.ENTRIES,)
    # ply 0: 81 points, no last move; ply 1: 80 (all but the stone); plies 2 and 3: 79
    assert seen.sum() == 81 + 80 + 79 + 79 and played.sum() == 3
    corner0 = 3 | 3 << 4 | 3 << 8 | 3 << 10 | 3 << 12
    # code 0 far from the last move: the 49 interior points; then all of them but 40 and its 8 neighbours; then also
    # without 10, which sees the white stone at 0; the same 39 after the pass
    assert seen[0] == 49 + 40 + 39 + 39
    assert played[0] == 1 and played[corner0] == 1 and seen[corner0] == 2    # 40 at ply 0; 0 at ply 1 (seen at plies 0, 1)
    # 41, east of the black stone: near with the opponent's stone west of it (ply 1), the mover's own stone (ply 2, the
    # last move far away), the opponent's after the pass (ply 3), where white plays it
    assert seen[NEAR | 2 << 4] == 1 and seen[1 << 4] == 1 and seen[2 << 4] == 1 and played[2 << 4] == 1
    assert played[NEAR | 2 << 4] == 0 and (seen[NEAR:].sum() == 8 + 3)       # near: 8 around 40 at ply 1, 1, 9, 10 at ply 2
    # the whole histogram against a recount by the definition
    want_seen, want_played = np.zeros_like(seen), np.zeros_like(played)
    g = go.Game()
    for mv in moves[0, :4].tolist():
        rec = records([g])
        for s in np.nonzero(RO.playable_host(rec)[0])[0].tolist():
            want_seen[slow_index(rec[0], s)] += 1
        if mv >= 0:
            want_played[slow_index(rec[0], mv)] += 1
            g.play_move(mv)
        else:
            g.play_pass()
    assert np.array_equal(seen, want_seen) and np.array_equal(played, want_played)
    # a move into the mover's own eye (self-play records may hold one) adds to seen only
    seen, played = PT.counts(records([go.Game(BOARD)]), np.array([[0]], np.int16), rules="host")
    assert seen.sum() == 1 and played.sum() == 0
    with pytest.raises(RuntimeError, match="illegal"):
        PT.counts(records([go.Game(BOARD)]), np.array([[1]], np.int16), rules="host")
    with pytest.raises(ValueError):
        PT.counts(records([go.Game()]), np.array([40], np.int16), rules="host")


def test_symmetrise_sums_the_orbits():
    rng = np.random.default_rng(2)
    seen, played = rng.integers(0, 50, PT.ENTRIES), rng.integers(0, 5, PT.ENTRIES)
    s, p = PT.symmetrise(seen, played)
    assert s.dtype == np.int64 and s.sum() >= seen.sum()
    idx = np.arange(PT.ENTRIES)
    for g in range(8):
        t = PT.transform_code(idx, g)
        assert np.array_equal(s[t], s) and np.array_equal(p[t], p)             # invariant under the group
    for i in (0, 5, 3 | 3 << 4 | 3 << 8 | 3 << 10 | 3 << 12, NEAR | 2 << 4, 54321, 131071):
        orbit = {int(PT.transform_code(i, g)) for g in range(8)}
        assert s[i] == sum(int(seen[j]) for j in orbit) and p[i] == sum(int(played[j]) for j in orbit), i
    assert s[0] == seen[0] and s[NEAR] == seen[NEAR]                            # the empty pattern is its own orbit
    # symmetric counts on the hand-made game: the four corners share their counts
    moves = np.array([[40, 0, go.PASS, 41]], np.int16)
    s, p = PT.symmetrise(*PT.counts(records([go.Game()]), moves, rules="host"))
    corners = [int(PT.codes_host(records([go.Game()]))[0, c]) for c in (0, 8, 72, 80)]
    assert len(set(corners)) == 4 and len({int(s[c]) for c in corners}) == 1 and all(p[c] == 1 for c in corners)
    table = PT.fit(records([go.Game()]), moves, rules="host")
    assert isinstance(table, PT.PatternTable) and table.array[0] == PT.weights(s, p)[0]


def test_the_table_file(tmp_path):
    rng = np.random.default_rng(3)
    table = PT.PatternTable(rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16))
    path = str(tmp_path / "table.npy")
    table.save(path)
    assert os.path.getsize(path) < 2 * PT.ENTRIES + 256
    assert np.array_equal(PT.PatternTable.load(path).array, table.array)
    assert np.array_equal(np.load(path), table.array)                          # a plain .npy
    assert np.array_equal(PT.as_table(path).array, table.array) and PT.as_table(table) is table and PT.as_table(None) is None
    assert (PT.PatternTable.constant(7).array == 7).all() and PT.PatternTable.constant(7).array.shape == (131072,)
    for bad in (np.zeros(PT.ENTRIES, np.int16), np.zeros(PT.ENTRIES, np.float32), np.zeros(65536, np.uint16),
                np.zeros((2, 65536), np.uint16), np.zeros(PT.ENTRIES + 1, np.uint16)):
        with pytest.raises(ValueError, match="pattern table"):
            PT.PatternTable(bad)
        np.save(str(tmp_path / "bad.npy"), bad)
        with pytest.raises(ValueError, match="pattern table"):
            PT.PatternTable.load(str(tmp_path / "bad.npy"))
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            PT.PatternTable.constant(bad)
    text = PT.show(table, 2)
    assert text.count("index") == 4 and "heaviest" in text and "lightest" in text
    assert PT.picture(NEAR | 2 << 4 | 3) == "\n".join([". # .", "O * .", ". . ."])


# ---- the callers ----------------------------------------------------------------------------------------------------------------
def test_native_mcts_takes_the_table(tmp_path):
    class Net:
        def engine(self):
            return _FakeEngine()

    rng = np.random.default_rng(4)
    table = PT.PatternTable(rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16))
    path = str(tmp_path / "t.npy")
    table.save(path)
    policy = lambda x: np.zeros((len(x), 81), np.float32)            # noqa: E731
    with pytest.raises(TypeError, match="playout_patterns"):
        NativeMCTS(Position(), policy, policy, playout_patterns=table)
    for given in (table, path):
        t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_patterns=given, playout_rules="host",
                       expand_thresh=1)
        assert isinstance(t.evaluator.patterns, PT.PatternTable) and np.array_equal(t.evaluator.patterns.array, table.array)
        t.rollout(6)
        assert t.root.value == 1.0 and t.choose().last_move == 38
        t.close()
    t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_rules="host")
    assert t.evaluator.patterns is None
    t.close()
    ev = RO.PlayoutEvaluator(_FakeEngine(), 3, seed=4, rules="host", patterns=table)
    recs = golden_records(4, 90)
    assert np.array_equal(ev(recs, 0)[1], RO.playout_value(recs, 3, 4, rules="host", patterns=table))


def test_command_lines(capsys):
    a = PT.parse_args(["fit", "-p", "w.bkw", "--games", "64", "--seed", "3", "-o", "t.npy"])
    assert (a.command, a.p, a.games, a.seed, a.o, a.records) == ("fit", "w.bkw", 64, 3, "t.npy", None)
    a = PT.parse_args(["fit", "-p", "w.bkw", "-o", "t.npy", "--records", "a", "b"])
    assert a.games == 4096 and a.records == ["a", "b"] and a.scale == 1024
    a = PT.parse_args(["show", "t.npy"])
    assert (a.command, a.table, a.n) == ("show", "t.npy", 8)
    for bad in (["fit", "-o", "t.npy"], ["fit", "-p", "w"], ["fit", "-p", "w", "-o", "t", "--games", "0"],
                ["fit", "-p", "w", "-o", "t", "--seed", "-1"], ["show"], ["show", "t", "-n", "0"], []):
        with pytest.raises(SystemExit):
            PT.parse_args(bad)
    assert gtp.parse_args([]).playout_patterns is None and match.parse_args([]).playout_patterns is None
    a = gtp.parse_args(["--playout-value", "64", "--playout-patterns", "t.npy"])
    assert a.playout_value == 64 and a.playout_patterns == "t.npy"
    a = match.parse_args(["--playout-value", "64", "--playout-patterns", "t.npy"])
    assert a.playout_value == 64 and a.playout_patterns == "t.npy"
    for bad in (["--playout-patterns", "t.npy"], ["--playout-patterns", "t.npy", "--playout-value", "0"],
                ["--playout-value", "8", "--playout-patterns", "t.npy", "-v", "v.pt"],
                ["--playout-value", "8", "--playout-patterns", "t.npy", "--simulate"],
                ["--playout-value", "8", "--playout-patterns", "t.npy", "--python-tree"]):
        with pytest.raises(SystemExit):
            gtp.parse_args(bad)
    for bad in (["--playout-patterns", "t.npy"],
                ["--playout-value", "8", "--playout-patterns", "t.npy", "--engine", "python -m oracle.gtp_cpu"]):
        with pytest.raises(SystemExit):
            match.parse_args(bad)
    a = RO._parse(["--sgf", "g.sgf", "--random", "--patterns", "t.npy"])
    assert a.random and a.patterns == "t.npy" and RO._parse(["--sgf", "g.sgf", "--random"]).patterns is None
    with pytest.raises(SystemExit):
        RO._parse(["--sgf", "g.sgf", "--patterns", "t.npy"])
    capsys.readouterr()


# ---- the declarations, the bindings, the build ------------------------------------------------------------------------------
def test_header_and_binding():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_PATTERN_ENTRIES\s+131072\b", src) and T.PATTERN_ENTRIES == PT.ENTRIES == 131072
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_pattern_codes\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*int32_t\s*\*\s*codes\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+bkt_pattern_playouts\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,\s*int\s+max_plies\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,"
                     r"\s*int32_t\s*\*\s*status\s*,\s*void\s*\*\s*stream\s*\)", code)
    res, args = T.SYMBOLS["bkt_pattern_playouts"]
    assert res is ctypes.c_int and len(args) == 11 and args[2] is ctypes.c_uint64 and args[1] is args[5] is ctypes.c_int
    same = T.SYMBOLS["bkt_random_playouts"][1]
    assert args[:4] == same[:4] and args[5:] == same[4:]                       # the same contract, the table put in
    res, args = T.SYMBOLS["bkt_pattern_codes"]
    assert res is ctypes.c_int and len(args) == 4 and args[1] is ctypes.c_int
    assert callable(T.pattern_playouts) and callable(T.pattern_codes)
    assert all(hasattr(PT, name) for name in PT.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_pattern_playouts and lib.bkt_pattern_codes and lib.bkt_random_playouts
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"-shared bk_train\.hip bk_train_bf16\.hip bk_playout_pat\.hip -o", make)
    assert '#include "bk_playout_mc.hip"' in open(os.path.join(CSRC, "bk_playout_pat.hip")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernels_build_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    for name in ("pattern_playouts_kernel", "pattern_codes_kernel", "random_playouts_kernel", "playout_step_kernel",
                 "play_moves_kernel", "area_score_kernel"):
        assert any(name in k for k in kernels), kernels
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(spills) == 2 * len(kernels) and len(scratch) == len(kernels)
    assert all(int(n) == 0 for _, n in spills), spills
    assert all(int(n) == 0 for n in scratch), scratch

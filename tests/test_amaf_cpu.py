"""CPU: the all-moves-as-first counts of the playouts and the search prior made of them, as far as they need no
GPU -- the declaration and the binding of bkt_amaf_counts, the host mirror against counts written out by hand,
playout_amaf and amaf_prior on the host rules, PlayoutEvaluator(prior=) through both step loops, the keywords and the
command lines, and the kernel's resources when compiled for gfx950."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, selfplay
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import REPO

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
PASS, NONE = go.PASS, RO.MOVE_NONE

# Black to move; black's only playable point is 38, which captures the white stone at 37; then both sides pass and black
# wins by 3.5: every playout is [38, pass, pass], whatever the draws.
BOARD = "".join([".XXXXOOO."] + ["XXXXXOOOO"] * 3 + ["XO.XXOOOO"] + ["XXXXXOOOO"] * 3 + ["XXXXXOOO."])

# records = 2, playouts = 3, max_plies = 8.  Even plies are the record's side to move.
HAND_MOVES = np.array([
    # record 0
    [5, 7, 7, PASS, 5, 81, 9, NONE],        # 5 counts once (plies 0 and 4); 7 was the opponent's first (ply 1): its recapture at
                                            # ply 2 does not count; a pass; 81 is ignored; 9 counts (ply 6); won
    [NONE] * 8,                             # nothing but the end marker; won, which changes nothing
    [0, 1, 2, 3, 4, 5, 6, 80],              # full to max_plies, no end marker: 0 2 4 6 count, 1 3 5 80 are the opponent's; lost
    # record 1
    [40, PASS, -3, 41, 42, 43, 44, 45],     # 40 counts; -3 ends the row as the marker does; lost
    [PASS, 40, 40, PASS, 41, PASS, 80, 7],  # 40 was the opponent's first; 41 (ply 4) and 80 (ply 6) count; 7 is the opponent's; won
    [40, 41, 81, 81, 12, 12, NONE, 3],      # 40 and 12 (ply 4) count; 41 is the opponent's; 3 stands behind the end; won
], np.int16)
HAND_WON = np.array([1, 1, 0, 0, 1, 1], np.uint8)
HAND_PLAYED = np.zeros((2, 81), np.int32)
HAND_WON_AT = np.zeros((2, 81), np.int32)
HAND_PLAYED[0, [5, 9, 0, 2, 4, 6]] = 1
HAND_WON_AT[0, [5, 9]] = 1
HAND_PLAYED[1, [40, 41, 80, 12]] = [2, 1, 1, 1]
HAND_WON_AT[1, [40, 41, 80, 12]] = 1


def records(games):
    return np.stack([np.frombuffer(bytes(g._pos), np.uint8) for g in games])


def three_records():
    """The board that needs no luck, the empty board, and a record whose last move is a pass."""
    passed = go.Game()
    passed.play_move(40)
    passed.play_pass()
    return records([go.Game(BOARD), go.Game(), passed])


def seeded_tables():
    """A pattern table and a tactics table over the whole uint16 range, as test_gpu_patterns.py and test_gpu_tactics.py
    build theirs."""
    rng = np.random.default_rng(17)
    w = rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16)
    w[rng.integers(0, PT.ENTRIES, 4096)] = 0
    w[rng.integers(0, PT.ENTRIES, 4096)] = 65535
    w[0], w[1 << 16] = 0, 65535
    t = np.random.default_rng(23).integers(0, 65536, TC.ENTRIES).astype(np.uint16)
    t[8], t[4], t[9], t[20] = 65535, 0, 65535, 0
    return PT.PatternTable(w), TC.TacticTable(t)


def same_amaf(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("value", "wins", "played", "won")) and a.n == b.n


# ---- 1. the declaration -------------------------------------------------------------------------------------------------------
def test_header_binding_and_all_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_amaf_counts\s*\(\s*const\s+int16_t\s*\*\s*moves\s*,\s*int\s+max_plies\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*int32_t\s*\*\s*played\s*,\s*int32_t\s*\*\s*won_at\s*,\s*void\s*\*\s*stream\s*\)", code)
    res, args = T.SYMBOLS["bkt_amaf_counts"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, I, P, I, I, P, P, P]
    assert callable(T.amaf_counts) and T.MAX_SAMPLE_ROWS == 1 << 24
    assert re.search(r"#define\s+BKT_MAX_SAMPLE_ROWS\s+\(1\s*<<\s*24\)", src)
    for name in ("Amaf", "amaf_counts_host", "amaf_prior", "playout_amaf"):
        assert name in RO.__all__ and hasattr(RO, name)
    assert all(hasattr(RO, name) for name in RO.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_amaf_counts
    # a translation unit of its own on the library's compile line, outside the text-include chain of bk_playout*.hip
    make = open(os.path.join(CSRC, "Makefile")).read()
    (line,) = [l for l in make.splitlines() if l.startswith("\t") and "-o $@" in l and "bk_playout_pat.hip" in l]
    assert "bk_playout_amaf.hip" in line.split()
    for name in ("bk_playout.hip", "bk_playout_mc.hip", "bk_playout_pat.hip", "bk_playout_tac.hip"):
        assert "bk_playout_amaf" not in open(os.path.join(CSRC, name)).read()


# ---- 2. the mirror against counts written out by hand ------------------------------------------------------------------------
def test_host_counts_equal_the_hand_written_ones():
    played, won_at = RO.amaf_counts_host(HAND_MOVES, HAND_WON, 2, 3)
    assert played.dtype == won_at.dtype == np.int32 and played.shape == won_at.shape == (2, 81)
    assert np.array_equal(played, HAND_PLAYED), np.nonzero(played != HAND_PLAYED)
    assert np.array_equal(won_at, HAND_WON_AT), np.nonzero(won_at != HAND_WON_AT)
    # the same rows as six records of one playout each: nothing crosses a row
    played1, won1 = RO.amaf_counts_host(HAND_MOVES, HAND_WON, 6, 1)
    assert np.array_equal(played1.reshape(2, 3, 81).sum(1), HAND_PLAYED)
    assert np.array_equal(won1.reshape(2, 3, 81).sum(1), HAND_WON_AT)
    assert not played1[1].any() and played1[2].sum() == 4 and not won1[2].any()
    for bad in ((HAND_MOVES, HAND_WON, 3, 3), (HAND_MOVES, HAND_WON[:5], 2, 3), (HAND_MOVES, HAND_WON, 0, 3),
                (HAND_MOVES[0], HAND_WON, 2, 3)):
        with pytest.raises(ValueError):
            RO.amaf_counts_host(*bad)


# ---- 3. playout_amaf on the host rules ----------------------------------------------------------------------------------------
def test_playout_amaf_on_the_host():
    recs, n = three_records(), 4
    a = RO.playout_amaf(recs, n, 3, rules="host")
    assert a.n == n and a.value.dtype == np.float32 and a.wins.dtype == a.played.dtype == a.won.dtype == np.int32
    assert a.value.shape == a.wins.shape == (3,) and a.played.shape == a.won.shape == (3, 81)
    value = RO.playout_value(recs, n, 3, rules="host")
    assert np.array_equal(a.value.view(np.int32), value.view(np.int32))
    assert np.array_equal(a.value, ((2 * a.wins - n) / np.float32(n)).astype(np.float32))
    assert (0 <= a.won).all() and (a.won <= a.played).all() and (a.played <= n).all() and (a.wins <= n).all()
    assert (a.won.max(1) <= a.wins).all()
    # the board that needs no luck: every playout is [38, pass, pass] and black wins it; no stone of the record but the
    # captured one at 37 ever leaves the board, and nobody plays where it stood
    want = np.zeros(81, np.int32)
    want[38] = n
    assert a.wins[0] == n and np.array_equal(a.played[0], want) and np.array_equal(a.won[0], want)
    occupied = recs[0, :81] != 0
    assert occupied.sum() == 77 and not a.played[0, occupied].any()
    # the empty board: the side to move opens somewhere in every playout, and most points get played by somebody
    assert a.played[1].sum() > n * 20 and (a.played[1] > 0).sum() > 40
    # a record's result is its own: the row and the rest of the batch do not enter
    order = [2, 0, 0, 1, 2]
    b = RO.playout_amaf(recs[order], n, 3, rules="host")
    for f in ("value", "wins", "played", "won"):
        assert np.array_equal(getattr(b, f), getattr(a, f)[order]), f
    assert not same_amaf(RO.playout_amaf(recs, n, 4, rules="host"), a)      # the seed does enter
    # with tables: their playouts, and again playout_value's value
    table, tactics = seeded_tables()
    for kw in (dict(patterns=table), dict(patterns=table, tactics=tactics)):
        t = RO.playout_amaf(recs, n, 3, rules="host", **kw)
        assert np.array_equal(t.value.view(np.int32), RO.playout_value(recs, n, 3, rules="host", **kw).view(np.int32))
        assert np.array_equal(t.played[0], want) and (t.won <= t.played).all() and (t.played <= n).all()
        assert not np.array_equal(t.played[1], a.played[1])
    with pytest.raises(ValueError):
        RO.playout_amaf(recs, 0, 3, rules="host")
    with pytest.raises(ValueError, match="rules"):
        RO.playout_amaf(recs, n, 3, rules="gnugo")


def test_a_stone_of_the_record_is_played_on_only_after_its_capture():
    """played > 0 on a point occupied at the record means the stone was captured in that playout; the counts say so by the
    history they are made of."""
    recs, n = three_records()[2:], 4
    a = RO.playout_amaf(recs, n, 3, rules="host")
    fin = RO.random_playouts(np.repeat(recs, n, 0), 3, counters=RO.value_counters(recs, n), rules="host")
    first = [(fin.moves[j] == 40).argmax() if (fin.moves[j] == 40).any() else -1 for j in range(n)]
    assert a.played[0, 40] == sum(1 for k in first if k >= 0 and k % 2 == 0)


# ---- 4. the prior -----------------------------------------------------------------------------------------------------------------
def _amaf(played, won, wins, n):
    return RO.Amaf(None, np.asarray(wins, np.int32), np.asarray(played, np.int32), np.asarray(won, np.int32), n)


def test_amaf_prior():
    ko = go.Game()
    for mv in (go.squash("D5"), go.squash("E5"), go.squash("E4"), go.squash("F4"), go.squash("E6"), go.squash("F6"),
               go.squash("A1"), go.squash("G5"), go.squash("F5")):
        ko.play_move(mv)
    recs = np.concatenate([three_records(), records([ko])])
    legal = RO.legal_host(recs)
    assert np.nonzero(legal[0])[0].tolist() == [0, 38] and legal[1].all() and legal[2].sum() == 80   # 0: black's own eye
    assert legal[3].sum() == 72 and not legal[3, go.squash("E5")] and recs[3, go.squash("E5")] == 0     # the ko point
    a = RO.playout_amaf(recs, 4, 3, rules="host")
    p = RO.amaf_prior(recs, a)
    assert p.dtype == np.float32 and p.shape == (4, 81)
    assert np.abs(p.astype(np.float64).sum(1) - 1).max() < 81 * 2.0 ** -24 and (p[~legal] == 0).all() and (p[legal] > 0).all()
    assert p[0, 38] == p[0, 0] == 0.5                                 # 38 won all it was played in; 0 stands at the win rate, 1
    # the formula, from the integers
    k, temp = 4.0, 0.1
    q = (a.won + k * (a.wins / 4.0)[:, None]) / (a.played + k)
    for r in range(4):
        e = np.where(legal[r], np.exp((q[r] - q[r][legal[r]].max()) / temp), 0.0)
        assert np.array_equal(p[r], (e / e.sum()).astype(np.float32)), r
    assert not np.array_equal(RO.amaf_prior(recs, a, k=1.0), p) and not np.array_equal(RO.amaf_prior(recs, a, temperature=1.0), p)
    # no counts: uniform over the legal points
    zero = _amaf(np.zeros((4, 81)), np.zeros((4, 81)), [0, 2, 4, 1], 4)
    u = RO.amaf_prior(recs, zero)
    for r in range(4):
        assert np.array_equal(u[r], np.where(legal[r], np.float32(1.0 / legal[r].sum()), np.float32(0))), r
    # no legal point: 1/81 everywhere
    full = np.frombuffer(bytes(go.Game(BOARD)._pos), np.uint8).copy()
    full[:81][full[:81] == 0] = 1                                     # a board without an empty point (no game reaches it)
    assert not RO.legal_host(full[None]).any()
    assert np.array_equal(RO.amaf_prior(full[None], _amaf(np.ones((1, 81)), np.zeros((1, 81)), [1], 4)),
                          np.full((1, 81), 1 / 81, np.float32))
    # at equal `played`, more wins give a higher prior; an unplayed point stands at the playouts' own win rate
    played, won = np.zeros((1, 81)), np.zeros((1, 81))
    played[0, [10, 11, 12]] = 8
    won[0, [10, 11, 12]] = [2, 5, 8]
    p = RO.amaf_prior(recs[1:2], _amaf(played, won, [8], 16))[0]
    assert p[10] < p[11] < p[12] and p[10] < p[13] < p[12] and len(set(p[13:].tolist())) == 1
    for kw in (dict(k=0), dict(k=-1.0), dict(temperature=0), dict(temperature=-0.5), dict(k=float("nan"))):
        with pytest.raises(ValueError):
            RO.amaf_prior(recs, a, **kw)
    with pytest.raises(ValueError):
        RO.amaf_prior(recs[:2], a)


# ---- 5. the evaluator ---------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """submit_positions / wait of a LeafEngine: priors that depend on the record alone."""
    device_id = 0

    def __init__(self):
        self.asked = 0

    def submit_positions(self, recs, logits=False, probs=True, value=True, n_policy=None):
        assert probs and not value and not logits and n_policy == len(recs)
        self.asked += 1
        h = np.ascontiguousarray(recs[:, 184:192]).view(np.uint64)[:, 0]
        x = ((h[:, None] >> (np.arange(81, dtype=np.uint64) % np.uint64(50))) & np.uint64(15)).astype(np.float32) + 1
        return x / x.sum(1, keepdims=True)

    def wait(self, ticket):
        return {"probs": ticket}


KW = dict(n_games=2, rollouts=5, expand_thresh=2, noise_weight=0.25, sample_plies=2, max_turns=5, cap=200, threads=1,
          eager_top=2, n_pools=1)


def test_playout_evaluator_with_a_prior():
    recs = three_records()
    same = lambda x: x                                                # noqa: E731
    # prior=0: today's results, and no history
    eng = _FakeEngine()
    p0, v0 = RO.PlayoutEvaluator(eng, 2, seed=4, rules="host", prior=0.0)(recs, 2)
    p_old, v_old = RO.PlayoutEvaluator(_FakeEngine(), 2, seed=4, rules="host")(recs, 2)
    assert np.array_equal(p0, p_old) and np.array_equal(v0, v_old) and eng.asked == 1
    assert np.array_equal(p0, selfplay.normalise_like_categorical(_FakeEngine().submit_positions(recs[:2], False, True, False, 2)))
    assert np.array_equal(v0, RO.playout_value(recs, 2, 4, rules="host"))
    # prior=1 without an engine
    ev = RO.PlayoutEvaluator(None, 2, seed=4, rules="host", prior=1.0)
    assert ev.wants_positions and not hasattr(ev, "engine") and ev.policy_engine is None
    p1, v1 = ev(recs, 2)
    assert p1.shape == (2, 81) and p1.dtype == np.float32 and v1.shape == (3,) and np.array_equal(v1, v0)
    assert (ev.positions, ev.batches) == (3, 1)
    prior = RO.amaf_prior(recs[:2], RO.playout_amaf(recs[:2], 2, 4, rules="host"))
    assert np.array_equal(p1, selfplay.normalise_like_categorical(prior)) and p1[0, 38] == 0.5
    assert np.array_equal(ev.finish(ev.submit(recs, 2), normalise=same)[0], prior)
    p, v = ev(recs, 0)
    assert p.shape == (0, 81) and np.array_equal(v, v0)
    eng = _FakeEngine()                                               # an engine that is there is not asked
    assert np.array_equal(RO.PlayoutEvaluator(eng, 2, seed=4, rules="host", prior=1.0)(recs, 2)[0], p1) and eng.asked == 0
    # in between: the documented mix
    eng = _FakeEngine()
    ev = RO.PlayoutEvaluator(eng, 2, seed=4, rules="host", prior=0.5)
    ph, vh = ev.finish(ev.submit(recs, 2), normalise=same)
    pi = _FakeEngine().submit_positions(recs[:2], False, True, False, 2)
    assert np.array_equal(ph, (0.5 * pi.astype(np.float64) + 0.5 * prior.astype(np.float64)).astype(np.float32))
    assert np.array_equal(vh, v0) and eng.asked == 1
    p, _ = RO.PlayoutEvaluator(eng, 2, seed=4, rules="host", prior=0.25, prior_k=1.0, prior_temperature=0.5)(recs, 2)
    other = RO.amaf_prior(recs[:2], RO.playout_amaf(recs[:2], 2, 4, rules="host"), k=1.0, temperature=0.5)
    assert np.array_equal(p, selfplay.normalise_like_categorical(
        (0.75 * pi.astype(np.float64) + 0.25 * other.astype(np.float64)).astype(np.float32)))
    # what is refused
    with pytest.raises(TypeError, match="engine"):
        RO.PlayoutEvaluator(None, 2, prior=0.5, rules="host")
    with pytest.raises(TypeError, match="engine"):
        RO.PlayoutEvaluator(None, 2, rules="host")
    for kw in (dict(prior=-0.1), dict(prior=1.5), dict(prior=1.0, prior_k=0), dict(prior=1.0, prior_temperature=0)):
        with pytest.raises(ValueError):
            RO.PlayoutEvaluator(_FakeEngine(), 2, rules="host", **kw)


def test_net_free_self_play_through_both_step_loops():
    runs = []
    for native in (True, False, True):
        ev = RO.PlayoutEvaluator(None, 2, seed=4, rules="host", prior=1.0)
        local, total = selfplay.self_play(ev, native_loop=native, **KW)
        assert local["native_loop"] is native and ev.batches > 0
        runs.append(local["games"])
    assert runs[0] == runs[1] == runs[2]
    assert len(runs[0]) == 2 and all(len(g["moves"]) > 0 for g in runs[0].values())
    ev = RO.PlayoutEvaluator(_FakeEngine(), 2, seed=4, rules="host")      # the priors do enter the games
    assert selfplay.self_play(ev, native_loop=True, **KW)[0]["games"] != runs[0]


# ---- 6. keywords and flags -----------------------------------------------------------------------------------------------------
def test_native_mcts_searches_without_a_network():
    t = NativeMCTS(Position(board=BOARD), None, None, playout_value=2, playout_prior=1.0, playout_rules="host",
                   expand_thresh=1)
    assert isinstance(t.evaluator, RO.PlayoutEvaluator) and t.evaluator.prior == 1.0 and t.evaluator.policy_engine is None
    assert t.policy_net is None and t.no_sim and t.value_net_weight == 1.0
    t.rollout(6)
    assert t.root.value == 1.0 and t.winrate() > 0.5
    assert t.choose().last_move == 38
    t.close()

    class Net:
        def engine(self):
            return _FakeEngine()

    t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_prior=0.5, playout_rules="host", expand_thresh=1)
    assert t.evaluator.prior == 0.5 and t.evaluator.policy_engine is not None
    t.rollout(4)
    assert t.choose().last_move == 38
    t.close()
    t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_rules="host", expand_thresh=1)
    assert t.evaluator.prior == 0.0 and t.playout_prior == 0.0
    t.close()
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(Position(), Net(), None, playout_prior=1.0)
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(Position(), None, None, playout_prior=1.0)
    with pytest.raises(TypeError, match="policy_net"):
        NativeMCTS(Position(), None, None, playout_value=2, playout_prior=0.5, playout_rules="host")
    with pytest.raises(TypeError, match="policy_net"):
        NativeMCTS(Position(), None, None, playout_value=2, playout_rules="host")
    with pytest.raises(ValueError):
        NativeMCTS(Position(), Net(), None, playout_value=2, playout_prior=1.5, playout_rules="host")
    with pytest.raises(RuntimeError, match="HIP backend"):           # a plain callable has no engine to mix with
        NativeMCTS(Position(), lambda x: np.zeros((len(x), 81), np.float32), None, playout_value=2, playout_prior=0.5)


def test_command_lines(capsys):
    assert gtp.parse_args([]).playout_prior == 0.0
    a = gtp.parse_args(["--playout-value", "64", "--playout-prior", "1", "-r", "400"])
    assert (a.playout_value, a.playout_prior, a.r) == (64, 1.0, 400)
    assert gtp.parse_args(["--playout-value", "8", "--playout-prior", "0.25"]).playout_prior == 0.25
    for bad in (["--playout-prior", "1"], ["--playout-value", "8", "--playout-prior", "1.5"],
                ["--playout-value", "8", "--playout-prior", "-0.5"], ["--playout-value", "8", "--playout-prior", "x"]):
        with pytest.raises(SystemExit):
            gtp.parse_args(bad)
    assert match.parse_args([]).playout_prior == 0.0
    a = match.parse_args(["--playout-value", "64", "--playout-prior", "1", "--games", "100"])
    assert (a.playout_value, a.playout_prior, a.games) == (64, 1.0, 100)
    for bad in (["--playout-prior", "0.5"], ["--playout-value", "8", "--playout-prior", "2"],
                ["--playout-value", "8", "--playout-prior", "1", "--engine", "python -m oracle.gtp_cpu"]):
        with pytest.raises(SystemExit):
            match.parse_args(bad)
    a = selfplay.parse_args([])
    assert (a.playout_value, a.playout_prior, a.playout_patterns, a.playout_tactics) == (0, 0.0, None, None)
    assert (a.games, a.rollouts, a.policy, a.value, a.out) == (512, 400, None, None, None)
    a = selfplay.parse_args(["--playout-value", "64", "--playout-prior", "1", "--out", "r/", "--games", "8"])
    assert (a.playout_value, a.playout_prior, a.out, a.games) == (64, 1.0, "r/", 8)
    a = selfplay.parse_args(["--playout-value", "16", "--playout-patterns", "p.npy", "--playout-tactics", "t.npy", "--policy", "p.pt"])
    assert (a.playout_patterns, a.playout_tactics, a.policy, a.playout_prior) == ("p.npy", "t.npy", "p.pt", 0.0)
    for bad in (["--playout-prior", "1"], ["--playout-patterns", "p.npy"], ["--playout-tactics", "t.npy"],
                ["--playout-value", "-1"], ["--playout-value", "8", "--value", "v.pt"],
                ["--playout-value", "8", "--host-encode"], ["--playout-value", "8", "--playout-prior", "1.1"],
                ["--playout-value", "8", "--playout-prior", "1", "--policy", "p.pt"]):
        with pytest.raises(SystemExit):
            selfplay.parse_args(bad)
    a = RO._parse(["--sgf", "g.sgf", "--random", "--amaf", "-n", "64"])
    assert a.amaf is True and a.random is True and a.n == 64 and RO._parse(["--sgf", "g.sgf", "--random"]).amaf is False
    for bad in (["--sgf", "g.sgf", "--amaf"], ["--sgf", "g.sgf", "--amaf", "-p", "w.bkw"]):
        with pytest.raises(SystemExit):
            RO._parse(bad)
    capsys.readouterr()


# ---- 7. the kernel's resources --------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_builds_alone_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_amaf.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    assert len(blocks) == 1 and "amaf_counts_kernel" in blocks[0].split()[0], [b.split()[0] for b in blocks]
    field = lambda pat: int(re.search(pat + r": (\d+)", blocks[0]).group(1))  # noqa: E731
    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field(r"SGPRs Spill") == 0 and field(r"VGPRs Spill") == 0, blocks[0]
    # two staging buffers of 4 rows x 1024 int16 and the waves' partial counts; registers that leave the SIMD full
    assert field(r"LDS Size \[bytes/block\]") == 2 * 4 * 1024 * 2 + 4 * 2 * 81 * 4, blocks[0]
    assert field(r" VGPRs") <= 64 and field(r"Occupancy \[waves/SIMD\]") == 8, blocks[0]

"""CPU: the Monte-Carlo value that needs no GPU -- the declaration and the binding of bkt_random_playouts, the integer
selection and the Philox words of the host mirror (rollout.random_playouts(rules="host")), whole host games, playout_value
as a pure function of the record, the board whose value needs no playout luck, PlayoutEvaluator through both step loops
on the host rules, the command lines, and the kernel's resources when compiled for gfx950."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, reinforce, selfplay
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN, REPO
from test_rollout_cpu import BOARD, check_finished_games, records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
_PP = ctypes.POINTER(go.Pos)


def golden_records(n, step=1):
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][::step][:n]
    return records([go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]) for r in pos])


def test_header_binding_and_all_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_MAX_PLAYOUT_PLIES\s+1024\b", src) and T.MAX_PLAYOUT_PLIES == 1024
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_random_playouts\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*int\s+max_plies\s*,\s*uint8_t\s*\*\s*over\s*,"
                     r"\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,\s*int32_t\s*\*\s*status\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    res, args = T.SYMBOLS["bkt_random_playouts"]
    assert res is ctypes.c_int and len(args) == 10 and args[2] is ctypes.c_uint64 and args[1] is args[4] is ctypes.c_int
    assert callable(T.random_playouts)
    for name in ("random_playouts", "playout_value", "PlayoutEvaluator", "finish_games", "rollout_score"):
        assert name in RO.__all__ and hasattr(RO, name)
    assert all(hasattr(RO, name) for name in RO.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_random_playouts and lib.bkt_playout_step


def test_integer_selection():
    draws = [0, 1, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF, 0x12345678]
    for n in range(1, 82):
        got = RO.select_index(np.array(draws, np.uint32), np.full(len(draws), n)).tolist()
        assert got == [((x >> 8) * n) >> 24 for x in draws], n
        assert all(0 <= i < n for i in got), n
        assert got[0] == 0 and got[7] == n - 1                       # the extreme draws reach both ends
        assert ((0xFFFFFFFF >> 8) * n) < 2 ** 32                     # the kernel's 32-bit product does not wrap
    assert RO.select_index(np.uint32(0xFFFFFFFF), 0) == 0            # no playable point: the row passes
    # uniform up to n * 2^-24: every rank of n = 81 gets floor or ceil of 2^24 / 81 of the 2^24 values of x0 >> 8
    counts = np.bincount(((np.arange(2 ** 24, dtype=np.uint64) * np.uint64(81)) >> np.uint64(24)).astype(np.int64), minlength=81)
    assert counts.min() >= 2 ** 24 // 81 and counts.max() <= 2 ** 24 // 81 + 1


def test_host_games_use_the_philox_words_and_the_selection():
    """Replay a host game: at ply k the move is the select_index-th playable point under the word x0 of
    reinforce.philox4x32_10 with key `seed` and counter (c0, c1 + k, c2, c3)."""
    seed = (7 << 32) | 5
    ctr = np.array([[3, 0xFFFFFFFE, 9, 2], [11, 5, 0, 7]], np.uint32).view(np.int32)      # word 1 of row 0 wraps at ply 2
    start = records([go.Game()] * 2)
    fin = RO.random_playouts(start, seed, counters=ctr, rules="host")
    assert fin.over.all() and fin.unfinished == 0 and not hasattr(fin, "min_margin")
    play, recs = reinforce._play_fn(), start.copy()
    tmp = (ctypes.c_uint8 * 81)()
    for g in range(2):
        for k in range(int(fin.plies[g])):
            c = ctr.view(np.uint32)[g].copy()
            c[1] = (int(c[1]) + k) & 0xFFFFFFFF
            x0 = int(reinforce.philox4x32_10(c[None], reinforce.seed_key(seed))[0, 0])
            pts = np.nonzero(RO.playable_host(recs[g:g + 1])[0])[0]
            want = go.PASS if len(pts) == 0 else int(pts[((x0 >> 8) * len(pts)) >> 24])
            assert fin.moves[g, k] == want, (g, k)
            assert play(recs[g].ctypes.data, want) == 0
            go.golib().bk_pos_liberties(ctypes.cast(recs[g].ctypes.data, _PP), tmp)
    assert np.array_equal(recs, fin.records)
    assert not np.array_equal(fin.moves[0, :20], fin.moves[1, :20])
    # not the lock-step sampler's games: finish_games(engine=None) keeps its float CDF and its bits
    old = RO.finish_games(start, None, seed, counters=ctr, rules="host")
    assert not np.array_equal(old.moves[:, :20], fin.moves[:, :20])


def test_host_games_end_as_games_do():
    start = np.concatenate([records([go.Game()] * 4), golden_records(8, 60)])
    before = start.copy()
    fin = RO.random_playouts(start, 11, rules="host")
    assert np.array_equal(start, before), "the caller's records changed"
    assert fin.over.sum() >= 10 and fin.unfinished == int((~fin.over).sum())
    assert fin.moves.dtype == np.int16 and fin.score.dtype == np.float32 and fin.owner.dtype == np.int8
    assert fin.plies[:4].min() > 60 and fin.plies.max() <= RO.MAX_PLIES
    check_finished_games(fin, before)
    assert np.array_equal(fin.owner, RO.owner_host(fin.records))
    again = RO.random_playouts(before, 11, rules="host")
    assert np.array_equal(again.moves, fin.moves) and np.array_equal(again.records, fin.records)
    # a row's game is its record's, its counters' and the seed's: a subset with its own counters plays the same games
    c = RO.default_counters(12, RO.record_turns(before))
    sub = RO.random_playouts(before[5:9], 11, counters=c[5:9], rules="host", history=False)
    assert sub.moves is None and np.array_equal(sub.records, fin.records[5:9]) and np.array_equal(sub.score, fin.score[5:9])
    # the cap: scored as it stands, counted as unfinished; a record whose last move is a pass ends with its first pass
    cut = RO.random_playouts(before[:4], 11, max_plies=30, rules="host")
    assert cut.unfinished == 4 and cut.plies.tolist() == [30] * 4 and np.array_equal(cut.moves, fin.moves[:4, :30])
    done = go.Game(BOARD)
    done.play_move(38)
    done.play_pass()
    one = RO.random_playouts(records([done]), 0, rules="host")
    assert one.moves.tolist() == [[go.PASS]] and one.over.all() and one.plies.tolist() == [1]
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="max_plies"):
            RO.random_playouts(before, 0, max_plies=bad, rules="host")
    with pytest.raises(ValueError, match="rules"):
        RO.random_playouts(before, 0, rules="gnugo")


def test_playout_value_is_a_function_of_the_record():
    recs = np.concatenate([golden_records(10, 50), records([go.Game(), go.Game(BOARD)])])
    v = RO.playout_value(recs, 6, 3, rules="host")
    assert v.dtype == np.float32 and v.shape == (12,) and (np.abs(v) <= 1).all()
    assert set(np.round((v * 6 + 6) / 2, 6).tolist()) <= set(range(7))           # (2 w - n) / n with w = 0 .. n
    perm = np.random.default_rng(0).permutation(12)
    assert np.array_equal(RO.playout_value(recs[perm], 6, 3, rules="host"), v[perm])
    assert np.array_equal(RO.playout_value(recs[3:8], 6, 3, rules="host"), v[3:8])
    twice = RO.playout_value(np.concatenate([recs[4:5], recs[:2], recs[4:5]]), 6, 3, rules="host")
    assert twice.tolist() == [v[4], v[0], v[1], v[4]]
    assert not np.array_equal(RO.playout_value(recs, 6, 4, rules="host"), v)      # the seed does enter
    c = RO.value_counters(recs[:2], 3).view(np.uint32)
    h = [int.from_bytes(bytes(recs[i, 184:192]), "little") for i in range(2)]
    assert c.tolist() == [[h[i] & 0xFFFFFFFF, 0, h[i] >> 32, 4 * j + 3] for i in range(2) for j in range(3)]
    with pytest.raises(ValueError):
        RO.playout_value(recs, 0, 3, rules="host")


def test_the_board_that_needs_no_luck():
    g = go.Game(BOARD)
    for seed in (0, 9):
        fin = RO.random_playouts(records([g] * 3), seed, rules="host")
        assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 3 and fin.score.tolist() == [3.5] * 3
    after = go.Game(BOARD)
    after.play_move(38)
    for n in (1, 8):
        assert RO.playout_value(records([g, after]), n, 5, rules="host").tolist() == [1.0, -1.0]   # black wins; white to move
    r = RO.rollout_score([g], None, n=4, seed=1, rules="host", one_launch=True)[0]
    assert r.score == 3.5 and r.black_win == 1.0 and r.stones("dead") == [37] and r.unfinished == 0


class _FakeEngine:
    """submit_positions / wait of a LeafEngine: priors that depend on the record alone."""
    device_id = 0

    def submit_positions(self, recs, logits=False, probs=True, value=True, n_policy=None):
        assert probs and not value and not logits and n_policy == len(recs)
        h = np.ascontiguousarray(recs[:, 184:192]).view(np.uint64)[:, 0]
        x = ((h[:, None] >> (np.arange(81, dtype=np.uint64) % np.uint64(50))) & np.uint64(15)).astype(np.float32) + 1
        return x / x.sum(1, keepdims=True)

    def wait(self, ticket):
        return {"probs": ticket}


def test_playout_evaluator_through_both_step_loops():
    ev = RO.PlayoutEvaluator(_FakeEngine(), 2, seed=4, rules="host")
    assert ev.wants_positions and not hasattr(ev, "engine") and ev.policy_engine is not None
    recs = records([go.Game(BOARD), go.Game()])
    probs, values = ev(recs, 1)
    assert probs.shape == (1, 81) and values.shape == (2,) and values[0] == 1.0 and (ev.positions, ev.batches) == (2, 1)
    assert np.array_equal(values, RO.playout_value(recs, 2, 4, rules="host"))
    probs, values = ev(recs, 0)
    assert probs.shape == (0, 81) and values.shape == (2,)
    kw = dict(n_games=2, rollouts=5, expand_thresh=2, noise_weight=0.25, sample_plies=2, max_turns=5, cap=200, threads=1,
              eager_top=2, n_pools=1)
    runs = []
    for native in (True, False, True):
        ev = RO.PlayoutEvaluator(_FakeEngine(), 2, seed=4, rules="host")
        local, total = selfplay.self_play(ev, native_loop=native, **kw)
        assert local["native_loop"] is native and ev.batches > 0
        runs.append(local["games"])
    assert runs[0] == runs[1] == runs[2]
    assert len(runs[0]) == 2 and all(len(g["moves"]) > 0 for g in runs[0].values())


def test_native_mcts_takes_the_keyword_and_refuses_what_does_not_fit():
    policy = lambda x: np.zeros((len(x), 81), np.float32)            # noqa: E731  (a plain callable: no HIP engine)
    with pytest.raises(RuntimeError, match="rollout scoring needs the HIP backend"):
        NativeMCTS(Position(), policy, None, playout_value=8)
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(Position(), policy, policy, playout_value=8)
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(Position(), policy, None, playout_value=8, no_sim=False)
    with pytest.raises(ValueError):
        NativeMCTS(Position(), policy, None, playout_value=-1)

    class Net:                                                       # what HipPolicyNet offers the keyword: engine()
        def engine(self):
            return _FakeEngine()

    t = NativeMCTS(Position(board=BOARD), Net(), None, playout_value=2, playout_seed=6, playout_rules="host",
                   expand_thresh=1)
    assert isinstance(t.evaluator, RO.PlayoutEvaluator) and (t.evaluator.playouts, t.evaluator.seed) == (2, 6)
    assert t.no_sim and t.value_net_weight == 1.0
    t.rollout(6)
    assert t.root.value == 1.0 and t.winrate() > 0.5                 # the root's own value: every playout is black's
    assert t.choose().last_move == 38
    t.close()
    # the playouts are scored with the tree's komi: black's 9 points of area lose against 9.5
    root = Position(board=BOARD)
    root.komi = 9.5
    t = NativeMCTS(root, Net(), None, playout_value=2, playout_rules="host", expand_thresh=1)
    assert t.evaluator.komi == 9.5
    t.rollout(2)
    assert t.root.value == -1.0
    t.komi = 5.5                                                     # as GTP's `komi` sets it
    assert t.evaluator.komi == 5.5
    t.close()


def test_command_lines(capsys):
    assert gtp.build_parser().parse_args([]).playout_value == 0
    a = gtp.parse_args(["--playout-value", "64", "-r", "400"])
    assert a.playout_value == 64 and a.r == 400 and a.v.endswith("value_synth.bkw")
    assert gtp.parse_args(["-v", "v.pt"]).v == "v.pt" and gtp.parse_args([]).playout_value == 0
    for bad in (["--playout-value", "8", "-v", "v.pt"], ["--playout-value", "8", "--simulate"],
                ["--playout-value", "8", "--python-tree"], ["--playout-value", "-1"], ["--rollout-score", "-1"]):
        with pytest.raises(SystemExit):
            gtp.parse_args(bad)
    assert "-v" in capsys.readouterr().err
    a = RO._parse(["--sgf", "g.sgf", "--random", "-n", "64"])
    assert a.random is True and a.n == 64 and a.p is None and RO._parse(["--sgf", "g.sgf"]).random is False
    with pytest.raises(SystemExit):
        RO._parse(["--sgf", "g.sgf", "--random", "-p", "w.bkw"])
    a = match.parse_args(["--playout-value", "64", "-r", "400", "--games", "100"])
    assert (a.playout_value, a.r, a.games, a.engine) == (64, 400, 100, None) and match.parse_args([]).playout_value == 0
    for bad in (["--playout-value", "8", "--engine", "python -m oracle.gtp_cpu"], ["--playout-value", "-1"]):
        with pytest.raises(SystemExit):                              # the flag configures the in-process engine only
            match.parse_args(bad)
    capsys.readouterr()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_builds_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_mc.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    for name in ("random_playouts_kernel", "playout_step_kernel", "play_moves_kernel", "area_score_kernel"):
        assert any(name in k for k in kernels), kernels
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(spills) == 2 * len(kernels) and len(scratch) == len(kernels)
    assert all(int(n) == 0 for _, n in spills), spills
    assert all(int(n) == 0 for n in scratch), scratch


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_playout_kernels_keep_their_register_and_lds_budget(tmp_path):
    """The three playout kernels are one ply loop (bk_playout_mc.hip's playouts<Draw>) around __noinline__ helpers that keep
    it within 128 VGPRs: 4 waves/SIMD.  LDS bytes per block: what the three separate kernels used before they shared it."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    for name, lds in (("random_playouts_kernel", 5088), ("pattern_playouts_kernel", 6128), ("tactical_playouts_kernel", 12832)):
        (block,) = [b for b in blocks if name in b.split()[0]]
        field = lambda pat: int(re.search(pat + r": (\d+)", block).group(1))  # noqa: E731
        assert field(r"Occupancy \[waves/SIMD\]") >= 4 and field(r" VGPRs") <= 128, block
        assert field(r"ScratchSize \[bytes/lane\]") == 0 and field(r"SGPRs Spill") == 0 and field(r"VGPRs Spill") == 0, block
        assert field(r"LDS Size \[bytes/block\]") <= lds, block

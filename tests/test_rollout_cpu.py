"""CPU: what playing games out and scoring them adds that needs no GPU -- the host mirror of finish_games
(rules="host", engine=None), the new symbols and declarations, the command lines, the GTP commands with a stubbed
scorer, and the step kernel's file compiled for gfx950 without spills."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import genvals, go, gtp, reinforce
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import Position
from conftest import REPO
from test_selfplay_cpu import FakeNets, _Wrap

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"

# The only playable point for either side is 38 (C5), where black captures the stone at 37 (B5): every other empty point
# is an own eye or suicide.  Raw area: 43 - (37 + 5.5) = 0.5; finished: 45 - (36 + 5.5) = 3.5.
BOARD = "".join([".XXXXOOO."] + ["XXXXXOOOO"] * 3 + ["XO.XXOOOO"] + ["XXXXXOOOO"] * 3 + ["XXXXXOOO."])


def records(games):
    return np.stack([np.frombuffer(bytes(g._pos), np.uint8) for g in games])


def check_finished_games(fin, start):
    """Every game that is over ended with two passes, and neither side had a playable point: not when it passed, and not
    in the final position -- except the point a ko forbade the first of the two passers, which the passes have set free
    (the side to move in the final position is that passer)."""
    lib, play = go.golib(), reinforce._play_fn()
    tmp = (ctypes.c_uint8 * 81)()
    for g in np.nonzero(fin.over)[0].tolist():
        n = int(fin.plies[g])
        assert n >= 2 and fin.moves[g, n - 2:n].tolist() == [go.PASS, go.PASS], g
        assert (fin.moves[g, n:] == RO.MOVE_NONE).all()
        rec = np.array(start[g:g + 1])
        p = ctypes.cast(rec.ctypes.data, ctypes.POINTER(go.Pos))
        for i, mv in enumerate(fin.moves[g, :n].tolist()):
            if i == n - 2:
                ko = int(p.contents.ko)
            if i >= n - 2:
                assert not RO.playable_host(rec).any(), (g, i)
            assert play(rec.ctypes.data, mv) == 0
            lib.bk_pos_liberties(p, tmp)
        assert np.array_equal(rec[0], np.asarray(fin.records[g])), g
        assert set(np.nonzero(RO.playable_host(rec)[0])[0].tolist()) <= ({ko} if ko >= 0 else set()), g
        assert play(rec.ctypes.data, go.PASS) == 0
        assert not RO.playable_host(rec).any(), g


def test_the_board_that_needs_no_network():
    g = go.Game(BOARD)
    assert g.area_score() == 0.5
    ok = RO.playable_host(records([g]))
    assert np.nonzero(ok[0])[0].tolist() == [38]
    for seed in (0, 7):
        fin = RO.finish_games(records([g] * 3), None, seed, rules="host")
        assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 3
        assert fin.over.all() and fin.plies.tolist() == [3] * 3 and fin.unfinished == 0
        assert fin.score.tolist() == [3.5] * 3 and fin.score.dtype == np.float32
        assert fin.owner[0, 37] == 1 and fin.owner[0, 38] == 1 and fin.owner[0, 8] == -1
    for n in (1, 8):
        r = RO.rollout_score([g], None, n=n, seed=1, rules="host")[0]
        assert r.score == 3.5 and r.black_win == 1.0 and r.mean_score == 3.5
        assert r.stones("dead") == [37] and r.stones("seki") == [] and len(r.stones("alive")) == 76
        assert r.status[38] is None and r.status[0] is None
    after = go.Game(BOARD)
    after.play_move(38)
    fin = RO.finish_games(records([after]), None, 0, rules="host")
    assert fin.moves.tolist() == [[go.PASS, go.PASS]] and fin.plies.tolist() == [2]
    assert fin.score[0] == np.float32(after.area_score()) == 3.5


def test_a_short_random_game_on_the_host():
    start = records([go.Game()] * 6)
    before = start.copy()
    fin = RO.finish_games(start, None, 11, rules="host")
    assert np.array_equal(start, before), "the caller's records changed"
    assert fin.unfinished == 0 and fin.over.all()
    assert fin.plies.min() > 60 and fin.plies.max() <= RO.MAX_PLIES
    check_finished_games(fin, before)
    # the history replays to the final records, and every move was playable when it was made
    play = reinforce._play_fn()
    recs = before.copy()
    tmp = (ctypes.c_uint8 * 81)()
    for g in range(len(recs)):
        for mv in fin.moves[g, :fin.plies[g]].tolist():
            if mv >= 0:
                assert RO.playable_host(recs[g:g + 1])[0, mv]
            assert play(recs[g].ctypes.data, mv) == 0
            go.golib().bk_pos_liberties(ctypes.cast(recs[g].ctypes.data, ctypes.POINTER(go.Pos)), tmp)
    assert np.array_equal(recs, fin.records)
    assert np.array_equal(fin.owner, RO.owner_host(fin.records))
    assert fin.score.tolist() == [float(fin.owner[g].sum()) - 5.5 for g in range(len(recs))]
    # deterministic per seed; the draws belong to the game, so a subset gives the same games only with its own counters
    again = RO.finish_games(before, None, 11, rules="host")
    assert np.array_equal(again.moves, fin.moves)
    other = RO.finish_games(before, None, 12, rules="host")
    assert not np.array_equal(other.moves[:, :40], fin.moves[:, :40])
    sub = RO.finish_games(before[2:4], None, 11, counters=RO.default_counters(6, np.zeros(6))[2:4], rules="host")
    assert np.array_equal(sub.moves[0, :sub.plies[0]], fin.moves[2, :fin.plies[2]])
    assert np.array_equal(sub.records, fin.records[2:4])
    # the cap: scored as it stands, counted as unfinished
    cut = RO.finish_games(before, None, 11, max_plies=30, rules="host")
    assert cut.unfinished == 6 and not cut.over.any() and cut.plies.tolist() == [30] * 6
    assert np.array_equal(cut.moves, fin.moves[:, :30])


def test_default_counters_and_arguments():
    c = RO.default_counters(3, [0, 41, 7]).view(np.uint32)
    assert c.tolist() == [[0, 0, 0, 2], [1, 41, 0, 2], [2, 7, 0, 2]]
    recs = records([go.Game()] * 2)
    with pytest.raises(ValueError, match="rules"):
        RO.finish_games(recs, None, 0, rules="gnugo")
    with pytest.raises(ValueError, match="uint8"):
        RO.finish_games(recs.astype(np.int32), None, 0, rules="host")
    with pytest.raises(ValueError, match="pair form"):
        RO.finish_games(recs, (None, None), 0, rules="host")
    with pytest.raises(ValueError, match="sides"):
        RO.finish_games(recs, None, 0, rules="host", sides=(1,))
    mixed = recs.copy()
    assert reinforce._play_fn()(mixed[1].ctypes.data, 40) == 0
    with pytest.raises(ValueError, match="parity"):
        RO.finish_games(mixed, (object(), object()), 0, rules="host", sides=(1,))
    assert RO.format_score(3.5) == "B+3.5" and RO.format_score(-12.0) == "W+12" and RO.format_score(0.0) == "0"


def test_header_and_binding_name_the_new_symbols():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_MOVE_NONE\s+\(-2\)", src) and T.MOVE_NONE == -2 == RO.MOVE_NONE
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_playout_step\s*\(\s*void\s*\*\s*pos\s*,\s*const\s+int32_t\s*\*\s*moves\s*,\s*int\s+batch\s*,"
                     r"\s*uint8_t\s*\*\s*over\s*,\s*int32_t\s*\*\s*status\s*,\s*uint8_t\s*\*\s*planes\s*,"
                     r"\s*uint8_t\s*\*\s*playable\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+bkt_sample_moves_masked\s*\(\s*const\s+float\s*\*\s*logits\s*,\s*const\s+uint8_t\s*\*\s*mask\s*,"
                     r"\s*size_t\s+mask_stride\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,\s*const\s+uint32_t\s*\*\s*counters\s*,"
                     r"\s*int32_t\s*\*\s*moves\s*,\s*float\s*\*\s*logp\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert len(T.SYMBOLS["bkt_playout_step"][1]) == 8 and len(T.SYMBOLS["bkt_sample_moves_masked"][1]) == 9
    assert T.SYMBOLS["bkt_sample_moves_masked"][1][2] is ctypes.c_size_t
    assert callable(T.playout_step) and callable(T.sample_moves_masked)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4
        assert lib.bkt_playout_step and lib.bkt_sample_moves_masked


def test_command_lines_take_the_new_flags(tmp_path, capsys):
    d = str(tmp_path)
    assert reinforce._parse(["-w", d]).finish is False and reinforce._parse(["-w", d, "--finish"]).finish is True
    ap = gtp.build_parser()
    assert ap.parse_args([]).rollout_score == 0 and ap.parse_args(["--rollout-score", "64"]).rollout_score == 64
    a = RO._parse(["--sgf", "g.sgf"])
    assert (a.n, a.move, a.p, a.seed, a.komi, a.device) == (256, None, None, 0, 5.5, 0)
    a = RO._parse(["--sgf", "g.sgf", "--move", "30", "-p", "w.bkw", "-n", "16", "--seed", "9"])
    assert (a.n, a.move, a.p, a.seed) == (16, 30, "w.bkw", 9)
    for bad in (["--sgf", "g.sgf", "-n", "0"], ["-n", "4"], ["--sgf", "g.sgf", "--move", "-1"]):
        with pytest.raises(SystemExit):
            RO._parse(bad)
    capsys.readouterr()
    import inspect
    assert inspect.signature(reinforce.play_games).parameters["finish"].default is False
    assert inspect.signature(genvals.generate).parameters["finish"].default is False
    assert inspect.signature(RO.finish_games).parameters["max_plies"].default == RO.MAX_PLIES == 400


def test_genvals_parses_finish(tmp_path):
    for name in ("policy_0.bkw", "policy_1.bkw"):
        (tmp_path / name).write_bytes(b"")
    assert genvals._parse(["-o", "x.csv", "-w", str(tmp_path)]).finish is False
    assert genvals._parse(["-o", "x.csv", "-w", str(tmp_path), "--finish"]).finish is True


def test_sgf_position(tmp_path):
    path = str(tmp_path / "g.sgf")
    go.write_sgf([40, 41, go.PASS, 30], path)
    assert RO.sgf_position(path).turn == 4 and RO.sgf_position(path, 2).turn == 2
    assert RO.sgf_position(path).board[30] == "O" and RO.sgf_position(path, 2).board[30] == "."


def _gtp(n, **kw):
    f = FakeNets()
    g = gtp.NativeGTP(Position(board=BOARD), _Wrap(f.policy), _Wrap(f.value, True), no_sim=True, time_lim=None,
                      n_rollouts=10, rollout_score=n, **kw)
    g.running = True
    return g


def test_gtp_commands_with_a_stubbed_scorer(monkeypatch):
    plain = _gtp(0)
    assert "final_status_list" not in plain.commands and plain.commands == gtp._GTPProtocol.commands
    assert plain.send("final_status_list dead") == "? unknown command 'final_status_list'\n\n"
    assert go.Game(BOARD).score() == -1.5                            # the reference's score of the board as it stands
    assert plain.send("final_score") == "= W+1.5\n\n"
    assert plain.send("known_command final_status_list") == "= false\n\n"

    g = _gtp(8, rollout_seed=5)
    assert g.commands[-1] == "final_status_list" and gtp._GTPProtocol.commands == plain.commands
    assert "final_status_list" in g.send("list_commands") and g.send("known_command final_status_list") == "= true\n\n"
    seen = []

    def scorer(self):
        seen.append((self.rollout_score_n, self.rollout_seed, self.root.board))
        return RO.rollout_score([self.root], None, n=self.rollout_score_n, seed=self.rollout_seed, rules="host")[0]

    monkeypatch.setattr(gtp._GTPProtocol, "_rollout_result", scorer)
    assert g.send("final_score") == "= B+3.5\n\n"
    assert g.send("7 final_status_list dead") == "=7 B5\n\n"
    assert g.send("final_status_list seki") == "= \n\n"
    alive = g.send("final_status_list alive")[2:].split()
    assert len(alive) == 76 and "B5" not in alive and "A2" in alive
    assert g.send("final_status_list") == "? usage: final_status_list <alive|dead|seki>\n\n"
    assert g.send("final_status_list white") == "? usage: final_status_list <alive|dead|seki>\n\n"
    assert seen and all(s == (8, 5, BOARD) for s in seen)


def test_gtp_refuses_rollout_scoring_without_a_hip_engine():
    g = _gtp(8)                                                      # the nets are plain callables: no HIP engine
    assert g.send("final_score") == "? rollout scoring needs the HIP backend\n\n"
    assert g.send("final_status_list dead") == "? rollout scoring needs the HIP backend\n\n"
    with pytest.raises(ValueError):
        _gtp(-1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_playout_kernels_build_without_spills(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(kernels) == 3 and len(spills) == 2 * len(kernels)
    assert any("playout_step_kernel" in k for k in kernels) and any("play_moves_kernel" in k for k in kernels)
    assert all(int(n) == 0 for _, n in spills), spills

"""-m gpu: the device Go rules (bkt_play_moves) against the host rules byte for byte, and the value-data generator
(bokego_amd/genvals.py) against its host-rules twin, go.Game, the samplers and itself."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import genvals as GV
from bokego_amd import go, nnet, train
from bokego_amd import reinforce as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_V, _I = ctypes.c_void_p, ctypes.c_int


def _fn(name, res, *args):
    return ctypes.cast(getattr(go.golib(), name), ctypes.CFUNCTYPE(res, *args))


def _host():
    return (_fn("bk_pos_play", _I, _V, _I), _fn("bk_pos_liberties", None, _V, _V),
            _fn("bk_pos_legal_moves", _I, _V, _V))


def _host_planes(recs):
    """bk_features_batch_u8 of the records (on a copy: it refreshes the cache it reads)."""
    c = np.ascontiguousarray(recs).copy()
    out = np.empty((len(c), 27, 9, 9), np.uint8)
    go.golib().bk_features_batch_u8(c.ctypes.data, len(c), 192, out.ctypes.data, 0)
    return out


def _step_both(recs, dpos, moves):
    """One ply on the host (bk_pos_play + bk_pos_liberties, in place on recs) and on the device; asserts that status,
    all 192 bytes of every record and the planes agree.  -> the host status codes."""
    play, libs, _ = _host()
    tmp = np.empty(81, np.uint8)
    want = np.zeros(len(recs), np.int32)
    base = recs.ctypes.data
    for i, m in enumerate(moves.tolist()):
        if m < 0:
            continue
        want[i] = play(base + 192 * i, m)
        if want[i] == 0:
            libs(base + 192 * i, tmp.ctypes.data)
    planes = torch.empty((len(recs), 27, 9, 9), dtype=torch.uint8, device=DEV)
    st = T.play_moves(dpos, torch.from_numpy(moves.astype(np.int32)).to(DEV), planes)
    got = dpos.cpu().numpy()
    np.testing.assert_array_equal(st.cpu().numpy(), want)
    bad = np.nonzero((got != recs).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} records differ, first row {bad[0]}: bytes {np.nonzero(got[bad[0]] != recs[bad[0]])[0]}"
    hp = _host_planes(recs)
    badp = np.nonzero((planes.cpu().numpy() != hp).reshape(len(recs), -1).any(1))[0]
    assert len(badp) == 0, f"{len(badp)} rows of planes differ, first row {badp[0]}"
    return want


def _record(board, turn=0):
    g = go.Game(board=board.replace(" ", ""), turn=turn)
    return np.frombuffer(bytes(g._pos), np.uint8).copy()


# ---- 1. rules, byte for byte -----------------------------------------------------------------------------------------------
def test_play_moves_random_games_byte_identical():
    G, plies = 4096, 110
    rng = np.random.default_rng(7)
    _, _, legal_moves = _host()
    recs = R.initial_positions(G)
    dpos = torch.from_numpy(recs.copy()).to(DEV)
    legal = np.empty(81, np.uint8)
    seen = {k: 0 for k in (-11, -12, -13, -14)}
    for ply in range(plies):
        moves = np.full(G, -1, np.int64)
        for i in range(G):
            a = recs.ctypes.data + 192 * i
            n = legal_moves(a, legal.ctypes.data)
            ko = int(recs[i, 164:166].view(np.int16)[0])
            board = recs[i, :81].view(np.int8)
            u = rng.random()
            if ko >= 0 and u < 0.3:
                moves[i] = ko                                        # ko recapture
            elif u < 0.05:
                occ = np.nonzero(board != 0)[0]
                moves[i] = rng.choice(occ) if len(occ) else -1       # occupied point
            elif u < 0.12:
                sui = np.nonzero((board == 0) & (legal == 0) & (np.arange(81) != ko))[0]
                moves[i] = rng.choice(sui) if len(sui) else -1       # suicide
            elif u < 0.13:
                moves[i] = 81 + int(rng.integers(0, 5))              # off the board
            elif u < 0.16:
                moves[i] = -1                                        # finished game
            elif n:
                moves[i] = rng.choice(np.nonzero(legal)[0])
        st = _step_both(recs, dpos, moves)
        for k in seen:
            seen[k] += int((st == k).sum())
    assert all(v > 0 for v in seen.values()), seen


def test_play_moves_crafted_positions():
    ko_board = (". X O . . . . . ."
                "X O . O . . . . ."
                ". X O . . . . . ." + "." * 54)
    double = (". O X . . . . . ."
              "O O X . . . . . ."
              "X X . . . . . . ." + "." * 54)
    recs = np.stack([_record(ko_board), _record(double)])
    dpos = torch.from_numpy(recs.copy()).to(DEV)
    # ply 0: no moves -- the planes of a record built from a board (cache invalid: the refresh is pending)
    _step_both(recs, dpos, np.array([-1, -1]))
    # black captures: a ko (one stone, every neighbour white), and a chain of 3 touching the move at two points
    assert _step_both(recs, dpos, np.array([11, 0])).tolist() == [0, 0]
    assert recs[0, 164:166].view(np.int16)[0] == 10                # the ko point
    assert recs[1, :81].view(np.int8)[[1, 9, 10]].tolist() == [0, 0, 0]
    assert recs[1, 81 + 10] != 0                                    # the captured points keep their stale count
    # white retakes the ko at once (refused); white plays on a point with a stale cached count (refresh skipped)
    assert _step_both(recs, dpos, np.array([10, 10])).tolist() == [go_code("ko"), 0]
    assert recs[1, 81 + 10] == 1                                    # stale: the stone's chain has more liberties
    assert _step_both(recs, dpos, np.array([80, 9])).tolist() == [0, 0]
    assert _step_both(recs, dpos, np.array([10, 1])).tolist() == [0, go_code("suicide")]   # white 1 + 10: no liberty
    assert _step_both(recs, dpos, np.array([40, 40])).tolist() == [0, 0]


def go_code(name):
    return {"ko": -11, "not_empty": -12, "suicide": -13, "off_board": -14}[name]


# ---- the generator ---------------------------------------------------------------------------------------------------------
def _perturbed(sd, seed=5, scale=0.05):
    """A second, distinct policy: every weight of sd times (1 + scale * N(0, 1)), seeded."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in sd.items():
        if v.dtype.is_floating_point and "running" not in k:
            v = v * torch.from_numpy(1 + scale * rng.standard_normal(tuple(v.shape))).to(v.dtype)
        out[k] = v
    return out


@pytest.fixture(scope="module")
def policies():
    sl_sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    return sl_sd, _perturbed(sl_sd)


@pytest.fixture(scope="module")
def engines(policies):
    sl = R.policy_engine(policies[0], 0, 512)
    rl = R.policy_engine(policies[1], 0, 512)
    yield sl, rl
    sl.close()
    rl.close()


@pytest.fixture(scope="module")
def device_run(engines):
    return GV.generate(*engines, 512, 512, 11, DEV, rules="device")


def test_device_rules_equal_host_rules(engines, device_run):
    host = GV.generate(*engines, 512, 512, 11, DEV, rules="host")
    assert device_run.rows == host.rows
    for k in ("r", "moves", "score", "kept", "game"):
        assert np.array_equal(getattr(device_run, k), getattr(host, k)), k
    assert len(device_run.rows) > 400


def test_replay_with_go_game(device_run):
    out = device_run
    rows = dict(zip(out.game.tolist(), out.rows))
    assert set(rows) == set(np.nonzero(out.kept)[0].tolist())
    for g in range(len(out.r)):
        hist, r = out.moves[g], int(out.r[g])
        if not out.kept[g]:
            assert hist[r] < 0
            continue
        game = go.Game()
        for ply, mv in enumerate(hist.tolist()):
            if mv < 0:
                assert all(m < 0 for m in hist[ply:]), "a game ends at its first ply without a move"
                assert ply > r and not any(game.is_legal(m) for m in range(81))
                break
            game.play_move(mv)                    # raises IllegalMove on an illegal move
            if ply == r:
                board, ko, last, turn, val = rows[g]
                assert (board, ko, last, turn) == (game.board, -1 if game.ko is None else game.ko, mv, r + 1)
        else:
            assert game.turn == GV.MAX_TURNS
        assert game.area_score() == pytest.approx(out.score[g])
        black_to_move = rows[g][3] % 2 == 0
        assert rows[g][4] == (1 if (out.score[g] > 0) == black_to_move else -1)


def _check_origin(eng, pairs, out, seed):
    """Re-evaluate the positions before (game, ply) with eng and draw with the documented counter."""
    planes = []
    for g, ply in pairs:
        game = go.Game()
        for mv in out.moves[g][:ply].tolist():
            game.play_move(mv)
        planes.append(game.features_u8())
    x = torch.from_numpy(np.stack(planes)).to(DEV)
    logits = eng.eval_device(x, logits=True, probs=False, value=False)["logits"]
    ctr = np.concatenate([GV.move_counters([g], ply) for g, ply in pairs])
    mv, _ = T.sample_moves(logits, x, seed, torch.from_numpy(ctr).to(DEV))
    want = np.array([out.moves[g][ply] for g, ply in pairs])
    np.testing.assert_array_equal(mv.cpu().numpy(), want)


def test_moves_come_from_their_policy(engines, device_run):
    out, rng = device_run, np.random.default_rng(3)
    games = rng.choice(np.nonzero(out.kept)[0], 64, replace=False)
    sl_pairs = [(int(g), int(rng.integers(0, out.r[g]))) for g in games]
    rl_pairs = [(int(g), int(rng.integers(out.r[g] + 1, GV.MAX_TURNS))) for g in games if out.r[g] + 1 < GV.MAX_TURNS]
    rl_pairs = [(g, p) for g, p in rl_pairs if out.moves[g][p] >= 0]
    _check_origin(engines[0], sl_pairs, out, 11)
    _check_origin(engines[1], rl_pairs, out, 11)
    # the random ply is the masked sampler's draw with the same counter layout
    x = []
    for g in games:
        game = go.Game()
        for mv in out.moves[g][:out.r[g]].tolist():
            game.play_move(mv)
        x.append(game.features_u8())
    x = torch.from_numpy(np.stack(x)).to(DEV)
    ctr = np.concatenate([GV.move_counters([g], out.r[g]) for g in games])
    mv, _ = T.sample_moves(GV.masked_logits(x), x, 11, torch.from_numpy(ctr).to(DEV))
    np.testing.assert_array_equal(mv.cpu().numpy(), [out.moves[g][out.r[g]] for g in games])


def test_masked_sampler_is_uniform_over_legal_points(device_run):
    from scipy.stats import chisquare
    out = device_run
    n = 20000
    for g in np.nonzero(out.kept)[0][:4]:
        game = go.Game()
        for mv in out.moves[g][:out.r[g]].tolist():
            game.play_move(mv)
        legal = np.array([game.is_legal(m) for m in range(81)])
        x = torch.from_numpy(np.repeat(game.features_u8()[None], n, 0)).to(DEV)
        ctr = torch.from_numpy(GV.move_counters(np.arange(n), int(g))).to(DEV)
        mv = T.sample_moves(GV.masked_logits(x), x, 99, ctr)[0].cpu().numpy()
        assert legal[mv].all()
        counts = np.bincount(mv, minlength=81)[legal]
        assert chisquare(counts).pvalue > 1e-4, counts


def test_same_seed_same_output_any_batch(engines, device_run):
    small = GV.generate(*engines, 512, 128, 11, DEV)
    assert small.rows == device_run.rows
    for k in ("r", "moves", "score"):
        assert np.array_equal(getattr(small, k), getattr(device_run, k)), k


def _cli(*args):
    r = subprocess.run([sys.executable, "-m", *args], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_cli_csv_is_byte_identical_and_trains_a_value_net(policies, tmp_path):
    rl = tmp_path / "rl.pt"
    torch.save({"model_state_dict": policies[1]}, rl)
    sl = os.path.join(GOLDEN, "policy_19.bkw")
    a, b = tmp_path / "a.csv", tmp_path / "b.csv"
    for p in (a, b):
        _cli("bokego_amd.genvals", "-o", str(p), "--sl", sl, "--rl", str(rl), "--games", "512", "--batch", "512",
             "--seed", "4")
    assert a.read_bytes() == b.read_bytes()
    rows = GV.read_rows(str(a))
    assert 400 < len(rows) <= 512

    out = tmp_path / "out"
    log = _cli("bokego_amd.train", "--values", str(a), "--net", "value", "-c", os.path.join(GOLDEN, "value_synth.bkw"),
               "-e", "20", "-b", "64", "--lr", "1e-3", "--seed", "1", "--out", str(out))
    lines = [json.loads(s) for s in log.strip().splitlines()]
    assert lines[-1]["value_loss"] < lines[0]["value_loss"], lines
    ck = torch.load(out / "value_20.pt")
    hv = nnet.HipValueNet(ck["model_state_dict"])
    ds = train.ValueRecordDataset([str(a)])
    v = hv(ds.planes[:64].astype(np.float32)).reshape(-1)
    v = torch.as_tensor(v)
    assert v.shape == (64,) and torch.isfinite(v).all()
    _cli("bokego_amd.selfplay", "--games", "2", "--rollouts", "8", "--max-turns", "6", "--value", str(out / "value_20.pt"))

"""-m gpu: bkt_area_score against bk_pos_area_score bit for bit, and the device-resident REINFORCE playouts
(reinforce.play_games(rules="device")) against the host-rules path field for field.  Every comparison is exact."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import genvals as GV
from bokego_amd import go, lockstep, train
from bokego_amd import reinforce as R
from conftest import GOLDEN
from test_reinforce_device_cpu import crafted_boards, host_scores, mirror_score, records_from_boards

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_V, _I = ctypes.c_void_p, ctypes.c_int


def _legal(rec):
    """bk_pos_legal_moves of one record -> the legal points."""
    fn = ctypes.cast(go.golib().bk_pos_legal_moves, ctypes.CFUNCTYPE(_I, _V, _V))
    rec, legal = np.ascontiguousarray(rec), np.empty(81, np.uint8)
    n = fn(rec.ctypes.data, legal.ctypes.data)
    pts = np.nonzero(legal)[0].tolist()
    assert n == len(pts)
    return pts


def _played(rec, mv):
    rec = np.ascontiguousarray(rec).copy()
    assert R._play_fn()(rec.ctypes.data, int(mv)) == 0
    return rec


@pytest.fixture(scope="module")
def policies():
    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    other = {k: (v + 0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(1), dtype=v.dtype)
                 if v.dtype.is_floating_point and "running_var" not in k else v) for k, v in sd.items()}
    return sd, other


@pytest.fixture(scope="module")
def engines(policies):
    a, b = R.policy_engine(policies[0], 0, 512), R.policy_engine(policies[1], 0, 512)
    yield a, b
    a.close()
    b.close()


# ---- 1. the score ----------------------------------------------------------------------------------------------------------
def _check_score(recs, komi=5.5):
    """T.area_score of the records: score equal to the host's float bit for bit, owner equal to the mirror (on at most the
    first 4096 distinct rows: the mirror is a Python flood fill), records untouched."""
    recs = np.ascontiguousarray(recs)
    d = torch.from_numpy(recs).to(DEV)
    score, owner = T.area_score(d, komi, owner=True)
    alone = T.area_score(d, komi)
    assert score.dtype == torch.float32 and tuple(score.shape) == (len(recs),)
    assert owner.dtype == torch.int8 and tuple(owner.shape) == (len(recs), 81)
    assert torch.equal(alone.view(torch.int32), score.view(torch.int32))
    assert np.array_equal(d.cpu().numpy(), recs), "the records changed"
    score, owner = score.cpu().numpy(), owner.cpu().numpy()
    uniq, first, inverse = np.unique(recs[:, :81], axis=0, return_index=True, return_inverse=True)
    want = host_scores(recs[first], komi)[inverse.reshape(-1)]
    bad = np.nonzero(score.view(np.int32) != want.view(np.int32))[0]
    assert len(bad) == 0, f"{len(bad)} scores differ, first row {bad[0]}: {score[bad[0]]} != {want[bad[0]]}"
    some = np.arange(len(uniq))[:4096]
    mirror = np.stack([mirror_score(uniq[i], komi)[1] for i in some])
    rows = np.nonzero(np.isin(inverse.reshape(-1), some))[0]
    badp = np.nonzero((owner[rows] != mirror[inverse.reshape(-1)[rows]]).any(1))[0]
    assert len(badp) == 0, f"{len(badp)} owner maps differ, first row {rows[badp[0]]}"
    return score, owner


def _golden_records():
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


def _final_records(games):
    """The records at the end of each game of a Playouts, replayed with bk_pos_play."""
    recs = R.initial_positions(len(games.length))
    play = R._play_fn()
    for g in range(len(recs)):
        for mv in games.moves[g, :games.length[g]].tolist():
            assert play(recs.ctypes.data + 192 * g, mv) == 0
    return recs


def test_area_score_golden_positions():
    recs = _golden_records()
    assert len(recs) > 500
    score, _ = _check_score(recs)
    assert len(np.unique(score)) > 10
    _check_score(recs[17:18])                                        # B = 1
    _check_score(recs[:2], komi=0.0)
    _check_score(recs[:100], komi=7.0)


def test_area_score_final_records_of_a_playout(engines):
    games = R.play_games(*engines, 2, 256, seed=13, rules="host")
    recs = _final_records(games)
    score, _ = _check_score(recs)
    assert np.array_equal(score > 0, games.black_wins)


def test_area_score_largest_batch():
    recs = _golden_records()
    _check_score(np.tile(recs, (65536 // len(recs) + 1, 1))[:65536])


def test_area_score_crafted_boards():
    c = crafted_boards()
    names = sorted(c)
    recs = records_from_boards(np.stack([c[n][0] for n in names]))
    score, owner = _check_score(recs)
    for i, n in enumerate(names):
        if c[n][1] is not None:
            assert score[i] == np.float32(c[n][1]), n
    assert score[names.index("empty")] == np.float32(-5.5) and not owner[names.index("empty")].any()
    assert score[names.index("two_eyes")] == np.float32(-86.5) and (owner[names.index("two_eyes")] == -1).all()
    own = owner[names.index("both_colours")].reshape(9, 9)
    assert (own[:, :4] == 1).all() and (own[:, 4] == 0).all() and (own[:, 5:] == -1).all()
    assert (owner[names.index("edge_and_black")] == 1).all()
    for k in (1, 2, 3, 4, 5):                                        # a workgroup holds three positions: every remainder
        _check_score(recs[:k])


def test_area_score_refuses_bad_arguments():
    lib = T.load()
    d = torch.from_numpy(R.initial_positions(4)).to(DEV)
    score = torch.full((4,), 123.0, dtype=torch.float32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for batch, komi in ((0, 5.5), (-1, 5.5), (65537, 5.5), (4, float("nan")), (4, float("inf"))):
        assert lib.bkt_area_score(d.data_ptr(), batch, komi, score.data_ptr(), None, s) == -1, (batch, komi)
    assert lib.bkt_area_score(None, 4, 5.5, score.data_ptr(), None, s) == -1
    assert lib.bkt_area_score(d.data_ptr(), 4, 5.5, None, None, s) == -1
    assert (score.cpu() == 123.0).all()                              # nothing was launched
    with pytest.raises(RuntimeError, match="BKT_ERR_ARG"):
        T.area_score(d, float("nan"))
    with pytest.raises(RuntimeError, match="BKT_ERR_ARG"):
        T.area_score(torch.empty((0, 192), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="BKT_ERR_ARG"):
        T.area_score(torch.zeros((65537, 192), dtype=torch.uint8, device=DEV))


# ---- 2. the same playouts ---------------------------------------------------------------------------------------------------
def _assert_same(dev, host):
    for k in ("moves", "length", "black_wins", "learner_black", "reward", "row_game"):
        a, b = getattr(dev, k), getattr(host, k)
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), k
    for k in ("planes", "played", "logp"):
        a, b = getattr(dev, k), getattr(host, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, k
    assert torch.equal(dev.planes, host.planes)
    assert torch.equal(dev.played, host.played)
    assert torch.equal(dev.logp.view(torch.int32), host.logp.view(torch.int32))


@pytest.mark.parametrize("W,b", [(2, 8), (3, 5), (16, 16)])
def test_device_playouts_equal_host_playouts(engines, W, b):
    kw = dict(seed=21 + W, iteration=3, epoch=2)
    dev = R.play_games(*engines, W, b, rules="device", **kw)
    host = R.play_games(*engines, W, b, rules="host", **kw)
    _assert_same(dev, host)
    assert len(dev.row_game) > 30 * W * b and dev.length.min() > 60  # whole games, not an early stop


def test_single_batch_and_timing_keys(engines):
    timing = {}
    dev = R.play_games(*engines, 1, 6, seed=5, rules="device", timing=timing)      # no learner-is-white slice
    _assert_same(dev, R.play_games(*engines, 1, 6, seed=5, rules="host"))
    assert set(timing) == {"engine", "sampler", "rules", "score", "download"}
    timing = {}
    R.play_games(*engines, 1, 6, seed=5, rules="host", timing=timing)
    assert set(timing) == {"host", "engine", "sampler"}


# ---- 3. games that end ------------------------------------------------------------------------------------------------------
def test_ended_games(engines):
    a_board = np.full(81, 2, np.uint8)
    a_board[[0, 80]] = 0                                             # (A) black has no legal point
    b_board = np.full(81, 1, np.uint8)
    b_board[[0, 40, 80]] = 0                                         # (B) black has three, then white has none
    rec_a, rec_b = records_from_boards(np.stack([a_board, b_board]))
    assert _legal(rec_a) == []
    assert _legal(rec_b) == [0, 40, 80]
    for mv in (0, 40, 80):
        assert _legal(_played(rec_b, mv)) == []
    empty = R.initial_positions(1)[0]
    W, b = 4, 4                                                      # batches 0, 2: the learner is black; 1, 3: white
    kinds = ["A", "B", "E", "E", "E", "A", "B", "E", "B", "E", "A", "E", "E", "B", "E", "A"]
    start = np.stack([{"A": rec_a, "B": rec_b, "E": empty}[k] for k in kinds])
    kw = dict(seed=4, iteration=1, epoch=5, start=start)
    dev = R.play_games(*engines, W, b, rules="device", **kw)
    host = R.play_games(*engines, W, b, rules="host", **kw)
    _assert_same(dev, host)
    for g, k in enumerate(kinds):
        rows = int((dev.row_game == g).sum())
        if k == "A":
            assert dev.length[g] == 0 and rows == 0 and (dev.moves[g] == go.PASS).all()
            assert not dev.black_wins[g]
        elif k == "B":
            assert dev.length[g] == 1 and dev.moves[g, 0] in (0, 40, 80) and (dev.moves[g, 1:] == go.PASS).all()
            assert rows == (1 if dev.learner_black[g] else 0)
            assert dev.black_wins[g]
        else:
            assert dev.length[g] > 60 and rows > 30
    assert {bool(dev.learner_black[g]) for g, k in enumerate(kinds) if k == "A"} == {True, False}
    assert {bool(dev.learner_black[g]) for g, k in enumerate(kinds) if k == "B"} == {True, False}


# ---- 4. nothing of the host rules per ply ----------------------------------------------------------------------------------
def test_device_path_runs_no_host_rules(engines, monkeypatch):
    calls = []

    def no_play():
        raise AssertionError("the device path asked for bk_pos_play")

    monkeypatch.setattr(lockstep, "_play_fn", no_play)
    real = lockstep.features_batch
    monkeypatch.setattr(lockstep, "features_batch", lambda recs, out: (calls.append(len(recs)), real(recs, out))[1])
    games = R.play_games(*engines, 2, 8, seed=9, rules="device")
    assert games.length.min() > 60 and len(calls) <= 1
    with pytest.raises(AssertionError):
        R.play_games(*engines, 2, 8, seed=9, rules="host")          # the patch does bite


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
def _pool(d):
    os.makedirs(d)
    shutil.copy(os.path.join(GOLDEN, "policy_19.bkw"), os.path.join(d, "policy_0.bkw"))
    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    g = torch.Generator().manual_seed(3)
    pert = {k: (v + 0.02 * v.abs().mean() * torch.randn(v.shape, generator=g) if k.endswith("weight") else v)
            for k, v in sd.items()}
    torch.save({"model_state_dict": pert}, os.path.join(d, "policy_1.pt"))


def test_cli_on_device_rules_equals_host_rules(tmp_path, capsys, monkeypatch):
    runs = []
    for name in ("device", "host"):
        d = str(tmp_path / name)
        _pool(d)
        stats = str(tmp_path / f"{name}.txt")
        if name == "host":
            play = R.play_games
            seen = []

            def host_rules(*args, **kw):                             # run_epoch with rules="host"
                seen.append(1)
                return play(*args, rules="host", **kw)

            monkeypatch.setattr(R, "play_games", host_rules)
        R.main(["-w", d, "-e", "1", "-n", "2", "-b", "4", "--workers", "4", "--seed", "7", "-f", stats])
        runs.append((torch.load(os.path.join(d, "policy_2.pt")), open(stats).read().splitlines()))
    capsys.readouterr()
    assert len(seen) == 2
    (a, la), (b, lb) = runs
    assert la == lb and len(la) == 3
    assert a["model_state_dict"].keys() == b["model_state_dict"].keys()
    assert all(torch.equal(a["model_state_dict"][k], b["model_state_dict"][k]) for k in a["model_state_dict"])
    sa, sb = a["optimizer_state_dict"]["state"], b["optimizer_state_dict"]["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i])
    start = torch.load(str(tmp_path / "device" / "policy_1.pt"))["model_state_dict"]
    assert not torch.equal(a["model_state_dict"]["conv.3.weight"], start["conv.3.weight"])


# ---- 6. genvals ------------------------------------------------------------------------------------------------------------
def test_genvals_scores_on_the_device(engines, monkeypatch):
    host = GV.generate(*engines, 256, 256, 11, DEV, rules="host")
    lib = go.golib()

    class NoScore:
        def __getattr__(self, name):
            if name == "bk_pos_area_score":
                raise AssertionError("the device rules scored on the host")
            return getattr(lib, name)

    monkeypatch.setattr(go, "golib", lambda: NoScore())
    dev = GV.generate(*engines, 256, 256, 11, DEV, rules="device")
    assert dev.score.dtype == host.score.dtype and np.array_equal(dev.score, host.score)
    assert dev.rows == host.rows and np.array_equal(dev.moves, host.moves)
    assert len(np.unique(dev.score)) > 10

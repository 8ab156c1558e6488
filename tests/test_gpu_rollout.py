"""-m gpu: bkt_playout_step and bkt_sample_moves_masked against the host rules and the host sampler, whole playouts to
the end of the game (rollout.finish_games) device against host, the board whose score needs no network, and the callers
(reinforce --finish, genvals --finish, GTP --rollout-score, the command line)."""
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
from bokego_amd import go, train
from bokego_amd import reinforce as R
from bokego_amd import rollout as RO
from conftest import GOLDEN, REPO
from test_rollout_cpu import BOARD, check_finished_games, records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_PP = ctypes.POINTER(go.Pos)
NONE = RO.MOVE_NONE


# ---- records ---------------------------------------------------------------------------------------------------------------
def _golden_records():
    """positions.json: records built from boards (liberty cache invalid)."""
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


def _played_records():
    """playouts.json replayed with bk_pos_play alone: records after every move, with the liberty cache as the moves left it
    (valid, a refresh pending at the last move)."""
    games = json.load(open(os.path.join(GOLDEN, "playouts.json")))["moves"][:48]
    play, out = R._play_fn(), []
    for moves in games:
        rec = R.initial_positions(1)
        for mv in moves:
            assert play(rec.ctypes.data, int(mv)) == 0
            out.append(rec[0].copy())
    return np.stack(out)


def _field(recs, off, dtype):
    return np.ascontiguousarray(recs[:, off:off + np.dtype(dtype).itemsize]).view(dtype)[:, 0]


def _legal_points(rec):
    buf = (ctypes.c_uint8 * 81)()
    go.golib().bk_pos_legal_moves(ctypes.cast(rec.ctypes.data, _PP), buf)
    return [s for s in range(81) if buf[s]]


@pytest.fixture(scope="module")
def pool():
    """The records of tests 1 and 2: golden and replayed ones, every record with a ko set that they hold, records that a
    capture-making move gives a ko, and copies whose last move is a pass."""
    recs = np.concatenate([_golden_records(), _played_records()])
    ko = recs[_field(recs, 164, np.int16) >= 0]
    passed = recs[::9].copy()
    for i in range(len(passed)):
        assert R._play_fn()(passed[i].ctypes.data, go.PASS) == 0
    out = np.concatenate([recs, ko, passed])
    assert (_field(out, 164, np.int16) >= 0).sum() >= 6 and (_field(out, 166, np.int16) == go.PASS).sum() > 100
    assert (out[:, 162] == 0).sum() > 500 and (out[:, 162] == 1).sum() > 500      # cache invalid / valid
    return np.ascontiguousarray(out)


def host_step(recs, moves, over):
    """bkt_playout_step's contract on the host -> (records, status, over, planes, playable)."""
    lib, play = go.golib(), R._play_fn()
    recs, over = recs.copy(), None if over is None else over.copy()
    status = np.zeros(len(recs), np.int32)
    tmp = (ctypes.c_uint8 * 81)()
    for b, mv in enumerate(moves.tolist()):
        if (over is not None and over[b]) or mv <= NONE:
            continue
        p = ctypes.cast(recs[b].ctypes.data, _PP)
        was_pass = p.contents.last_move == go.PASS
        rc = play(recs[b].ctypes.data, mv)
        status[b] = rc
        if rc == 0:
            lib.bk_pos_liberties(p, tmp)
            if mv == go.PASS and was_pass and over is not None:
                over[b] = 1
    planes = np.empty((len(recs), 27, 9, 9), np.uint8)
    scratch = recs.copy()                                            # the encoder refreshes the cache of what it reads
    lib.bk_features_batch_u8(scratch.ctypes.data, len(recs), 192, planes.ctypes.data, 0)
    return recs, status, over, planes, RO.playable_host(recs).astype(np.uint8)


def device_step(recs, moves, over, want_planes=True, want_playable=True):
    B = len(recs)
    d = torch.from_numpy(np.ascontiguousarray(recs)).to(DEV)
    d_over = None if over is None else torch.from_numpy(over.copy()).to(DEV)
    planes = torch.full((B, 27, 9, 9), 99, dtype=torch.uint8, device=DEV) if want_planes else None
    playable = torch.full((B, 81), 99, dtype=torch.uint8, device=DEV) if want_playable else None
    status = T.playout_step(d, torch.from_numpy(moves.astype(np.int32)).to(DEV), d_over, planes, playable)
    return (d.cpu().numpy(), status.cpu().numpy(), None if over is None else d_over.cpu().numpy(),
            None if planes is None else planes.cpu().numpy(), None if playable is None else playable.cpu().numpy())


def _compare(recs, moves, over, **kw):
    got, want = device_step(recs, moves, over, **kw), host_step(recs, moves, over)
    bad = np.nonzero((got[0] != want[0]).any(1))[0]
    assert len(bad) == 0, (f"{len(bad)} records differ, first row {bad[0]} move {moves[bad[0]]} at bytes "
                           f"{np.nonzero(got[0][bad[0]] != want[0][bad[0]])[0][:8]}")
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:8]
    if over is not None:
        assert np.array_equal(got[2], want[2]), np.nonzero(got[2] != want[2])[0][:8]
    if got[3] is not None:
        badp = np.nonzero((got[3] != want[3]).reshape(len(recs), -1).any(1))[0]
        assert len(badp) == 0, f"{len(badp)} plane sets differ, first row {badp[0]} move {moves[badp[0]]}"
    if got[4] is not None:
        badq = np.nonzero((got[4] != want[4]).any(1))[0]
        assert len(badq) == 0, f"{len(badq)} playable sets differ, first row {badq[0]} move {moves[badq[0]]}"
    return want


def _mixed_moves(recs, rng):
    """A point move, a pass, BKT_MOVE_NONE (or below), or an over flag on every row, by turns."""
    moves = np.full(len(recs), NONE, np.int32)
    over = np.zeros(len(recs), np.uint8)
    for i in range(len(recs)):
        kind = i % 5
        pts = _legal_points(recs[i])
        if kind in (0, 1) and pts:
            moves[i] = pts[int(rng.integers(len(pts)))]
        elif kind in (0, 1, 2):
            moves[i] = go.PASS
        elif kind == 3:
            moves[i] = NONE - int(rng.integers(3))
        else:
            over[i] = 1
            moves[i] = pts[0] if pts and i % 2 else go.PASS
    return moves, over


# ---- 1. the step --------------------------------------------------------------------------------------------------------------
def test_step_is_the_host_rules_on_every_kind_of_row(pool):
    rng = np.random.default_rng(1)
    moves, over = _mixed_moves(pool, rng)
    ko = np.nonzero(_field(pool, 164, np.int16) >= 0)[0]
    bad = int(np.argmax((pool[:, :81] != 0).sum(0)))                 # a point that is often occupied ...
    illegal = np.setdiff1d(np.nonzero(pool[:, bad] != 0)[0], ko)[:3]
    assert len(illegal) == 3
    moves[illegal], over[illegal] = bad, 0
    moves[ko[::2]], over[ko[::2]] = _field(pool, 164, np.int16)[ko[::2]], 0       # ... and retaking a ko; the others pass
    moves[ko[1::2]], over[ko[1::2]] = go.PASS, 0
    want = _compare(pool, moves, over)
    assert (want[1][illegal] == -12).all() and (want[1][ko[::2]] == -11).all() and set(np.unique(want[1])) <= {0, -11, -12}
    assert np.array_equal(want[0][illegal], pool[illegal])
    assert (want[2] > over).sum() > 10, "no row ended by a second pass"
    was_pass = _field(pool, 166, np.int16) == go.PASS
    assert np.array_equal(want[2] > over, (moves == go.PASS) & (over == 0) & was_pass)
    assert ((moves >= 0) & (want[1] == 0) & (over == 0)).sum() > 200
    assert np.array_equal(want[0][over != 0], pool[over != 0])       # an over row is untouched whatever its move
    _compare(pool, moves, None)                                      # over NULL: nothing ends, the over rows play
    _compare(pool, moves, over, want_planes=False)
    _compare(pool, moves, over, want_playable=False)
    _compare(pool, moves, None, want_planes=False, want_playable=False)


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 7])
def test_step_small_batches(pool, batch):
    """Three positions per workgroup: every remainder, with each kind of row in each place."""
    rows = np.concatenate([np.nonzero(_field(pool, 166, np.int16) == go.PASS)[0][:2],
                           np.nonzero(_field(pool, 164, np.int16) >= 0)[0][:2], [5, 700, 811]])
    base = pool[rows]
    pts = [_legal_points(r) for r in base]
    moves = np.array([go.PASS, pts[1][0], go.PASS, int(_field(base, 164, np.int16)[3]), NONE, go.PASS, pts[6][-1]], np.int32)
    over = np.array([0, 0, 0, 0, 0, 1, 0], np.uint8)
    for shift in range(7):
        idx = np.roll(np.arange(7), shift)[:batch]
        _compare(base[idx], moves[idx], over[idx])
        _compare(base[idx], moves[idx], None, want_planes=shift % 2 == 0, want_playable=shift % 2 == 1)


def test_step_refuses_bad_arguments():
    lib = T.load()
    d = torch.from_numpy(R.initial_positions(4)).to(DEV)
    mv = torch.full((4,), 40, dtype=torch.int32, device=DEV)
    st = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for batch in (0, -1, 65537):
        assert lib.bkt_playout_step(d.data_ptr(), mv.data_ptr(), batch, None, st.data_ptr(), None, None, s) == -1
    assert lib.bkt_playout_step(None, mv.data_ptr(), 4, None, st.data_ptr(), None, None, s) == -1
    assert lib.bkt_playout_step(d.data_ptr(), None, 4, None, st.data_ptr(), None, None, s) == -1
    assert lib.bkt_playout_step(d.data_ptr(), mv.data_ptr(), 4, None, None, None, None, s) == -1
    assert (st.cpu() == 77).all() and np.array_equal(d.cpu().numpy(), R.initial_positions(4))


# ---- 2. the playable set ------------------------------------------------------------------------------------------------------
def test_playable_set_on_the_eye_boards(pool):
    z = np.load(os.path.join(GOLDEN, "possible_eye.npz"))
    games = [go.Game(board="".join(".XO"[c] for c in b), turn=t) for b in z["boards"] for t in (0, 1)]
    recs = np.concatenate([records(games), pool])
    assert len(z["boards"]) == 1392 and len(recs) > 2 * 1392 + 500
    lib, own_eyes = go.golib(), 0
    buf = (ctypes.c_uint8 * 81)()
    for i in range(2 * 1392):                                         # counted on the host: legal points that are own eyes
        p = ctypes.cast(recs[i].ctypes.data, _PP)
        lib.bk_pos_legal_moves(p, buf)
        own_eyes += sum(1 for s in range(81) if buf[s] and lib.bk_pos_possible_eye(p, s) == 1 + (i & 1))
    assert own_eyes > 500, own_eyes
    want = RO.playable_host(recs).astype(np.uint8)
    d = torch.from_numpy(recs).to(DEV)
    playable = torch.full((len(recs), 81), 99, dtype=torch.uint8, device=DEV)
    status = T.playout_step(d, torch.full((len(recs),), NONE, dtype=torch.int32, device=DEV), None, None, playable)
    assert not status.any() and np.array_equal(d.cpu().numpy(), recs)
    got = playable.cpu().numpy()
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first {bad[0]} at points {np.nonzero(got[bad[0]] != want[bad[0]])[0]}"


# ---- 3. the sampler -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    e = R.policy_engine(train.load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 512)
    yield e
    e.close()


def _draw_counters(n, tag):
    c = np.zeros((n, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 3] = np.arange(n), 3, tag
    return c.view(np.int32)


@pytest.mark.parametrize("batch", [1, 4, 5, 257])
def test_masked_sampler(engine, batch):
    feats = np.load(os.path.join(GOLDEN, "playouts.npz"))["features"].astype(np.uint8)
    rows = np.arange(batch) % len(feats)
    planes = torch.from_numpy(feats[rows]).to(DEV)
    logits = torch.cat([engine.eval_device(planes[s:s + 256], logits=True, probs=False, value=False)["logits"]
                        for s in range(0, batch, 256)])
    seed = 0xABCDEF0123456789
    ctr = _draw_counters(batch, 9)
    d_ctr = torch.from_numpy(ctr).to(DEV)
    # the legal plane through the masked entry point: the bits of bkt_sample_moves
    mv0, lp0 = T.sample_moves(logits, planes, seed, d_ctr)
    mv1 = torch.full((batch,), -9, dtype=torch.int32, device=DEV)
    lp1 = torch.full((batch,), -9.0, dtype=torch.float32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    assert T.load().bkt_sample_moves_masked(logits.data_ptr(), planes.data_ptr() + 5 * 81, 2187, batch, seed,
                                            d_ctr.data_ptr(), mv1.data_ptr(), lp1.data_ptr(), s) == 0
    assert torch.equal(mv0, mv1) and torch.equal(lp0.view(torch.int32), lp1.view(torch.int32))
    # random masks, empty and single-point rows among them, against the float64 mirror
    rng = np.random.default_rng(batch)
    mask = (rng.random((batch, 81)) < rng.random((batch, 1))).astype(np.uint8)
    mask[::7] = 0
    single = np.arange(batch)[3::7]
    mask[single] = 0
    mask[single, rng.integers(81, size=len(single))] = 1
    got, glp = T.sample_moves_masked(logits, torch.from_numpy(mask).to(DEV), seed, d_ctr)
    got, glp, lg = got.cpu().numpy(), glp.cpu().numpy(), logits.cpu().numpy()
    u = R.uniform(R.philox4x32_10(ctr.view(np.uint32), R.seed_key(seed))[:, 0])
    want, wlp = R.sample_host(lg, mask != 0, u)
    near = R.cdf_margin(lg, u) < 1e-5
    diff = got != want
    assert near.mean() <= 0.005 or batch < 200 and near.sum() <= 1
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:10]
    assert np.abs(glp[~diff] - wlp[~diff]).max() <= 1e-5
    assert (got[::7] == -1).all() and (glp[::7] == 0).all()
    assert np.array_equal(got[single], np.argmax(mask[single], 1))
    ok = got >= 0
    assert (mask[np.arange(batch)[ok], got[ok]] != 0).all() and (mask[~ok] == 0).all()


# ---- 4. whole playouts ----------------------------------------------------------------------------------------------------------
GAMES, SEED = 64, 2024
# A move of the device and of the float64 mirror can differ only where u * S lies on a boundary of the CDF: the fp32 prefix
# sums are off by a few 1e-7 of S, there are 81 boundaries, so a draw differs with probability about 2 * 3e-7 * 81 = 5e-5 and
# the ~10^4 draws of 64 games hold 0.5 such draws on average (P(more than 3) < 0.2 %).  A game that differs must hold a draw
# within reinforce.cdf_margin < 1e-5 of a boundary (the rule of the sampler's own test), and at most 3 games may differ.
MAX_DIFFERING_GAMES = 3


@pytest.fixture(scope="module")
def ply40():
    """64 records at ply 40: uniformly random eye-safe games from the empty board, cut after 40 plies (host rules)."""
    fin = RO.finish_games(R.initial_positions(GAMES), None, 40, max_plies=40, rules="host")
    assert (RO.record_turns(fin.records) == 40).all() and not fin.over.any()
    return fin.records


def _same_playouts(dev, host):
    assert isinstance(dev.records, torch.Tensor) and dev.records.is_cuda
    L = max(dev.moves.shape[1], host.moves.shape[1])
    pad = lambda m: np.pad(m, ((0, 0), (0, L - m.shape[1])), constant_values=NONE)  # noqa: E731
    differs = ((pad(dev.moves) != pad(host.moves)).any(1) | (dev.records.cpu().numpy() != host.records).any(1)
               | (dev.over != host.over) | (dev.plies != host.plies) | (dev.score != host.score)
               | (dev.owner != host.owner).any(1))
    assert not (differs & (host.min_margin >= 1e-5)).any(), np.nonzero(differs & (host.min_margin >= 1e-5))[0]
    assert differs.sum() <= MAX_DIFFERING_GAMES, differs.sum()
    return differs


@pytest.mark.parametrize("with_engine", [True, False])
def test_whole_playouts_device_against_host(engine, ply40, with_engine):
    eng = engine if with_engine else None
    host = RO.finish_games(ply40, eng, SEED, rules="host")
    dev = RO.finish_games(ply40, eng, SEED)
    print(f"engine={with_engine}: plies mean {host.plies.mean():.1f} max {host.plies.max()}, unfinished {host.unfinished}, "
          f"black wins {int((host.score > 0).sum())}/{GAMES}")
    differs = _same_playouts(dev, host)
    assert host.unfinished == 0 and dev.unfinished == int((~dev.over).sum())
    assert (dev.over | differs).all()
    assert host.plies.max() < RO.MAX_PLIES
    check_finished_games(host, ply40)
    dev.records = dev.records.cpu().numpy()
    check_finished_games(dev, ply40)
    assert dev.score.dtype == np.float32 and dev.owner.dtype == np.int8 and dev.moves.dtype == np.int16
    assert np.array_equal(dev.score, dev.owner.sum(1).astype(np.float32) - np.float32(5.5))
    # from a device tensor, and again: the same bits
    again = RO.finish_games(torch.from_numpy(ply40).to(DEV), eng, SEED)
    assert np.array_equal(again.moves, dev.moves) and np.array_equal(again.records.cpu().numpy(), dev.records)
    # the draws belong to the game: a slice with its own counters plays the same games
    sub = RO.finish_games(ply40[10:23], eng, SEED, counters=RO.default_counters(GAMES, np.full(GAMES, 40))[10:23])
    n = sub.moves.shape[1]
    assert np.array_equal(sub.records.cpu().numpy(), dev.records[10:23])
    assert np.array_equal(sub.moves, dev.moves[10:23, :n]) and (dev.moves[10:23, n:] == NONE).all()


def test_pair_form_and_the_cap(engine, ply40):
    one = RO.finish_games(ply40, engine, SEED)
    for n0 in (0, 20, GAMES):
        two = RO.finish_games(ply40, (engine, engine), SEED, sides=(n0,))
        assert np.array_equal(two.moves, one.moves) and torch.equal(two.records, one.records)
        assert np.array_equal(two.score, one.score) and np.array_equal(two.over, one.over)
    odd = ply40.copy()
    assert R._play_fn()(odd[3].ctypes.data, go.PASS) == 0
    with pytest.raises(ValueError, match="parity"):
        RO.finish_games(odd, (engine, engine), SEED, sides=(20,))
    assert RO.finish_games(odd, engine, SEED).unfinished == 0         # the single form takes any mix of turns
    cut = RO.finish_games(ply40, engine, SEED, max_plies=20)
    assert cut.unfinished == GAMES and cut.plies.tolist() == [20] * GAMES and np.array_equal(cut.moves, one.moves[:, :20])
    host_area = np.array([go.golib().bk_pos_area_score(ctypes.cast(r.ctypes.data, _PP), 5.5)
                          for r in cut.records.cpu().numpy()], np.float32)
    assert np.array_equal(cut.score, host_area)                      # scored as it stands


@pytest.mark.parametrize("pair", [False, True])
def test_an_engine_smaller_than_the_batch(ply40, pair):
    """Seven records through an engine of max_batch 4 (the rows of a slice go to it four at a time) play the games of the
    same call through an engine of max_batch 8, field for field: once in the single form, once in the pair form."""
    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    fins = []
    for max_batch in (4, 8):
        e = R.policy_engine(sd, 0, max_batch)
        try:
            fins.append(RO.finish_games(ply40[:7], (e, e), SEED, sides=(3,), max_plies=40) if pair else
                        RO.finish_games(ply40[:7], e, SEED, max_plies=40))
        finally:
            e.close()
    small, big = fins
    assert torch.equal(small.records, big.records) and small.unfinished == big.unfinished
    for k in ("moves", "over", "plies", "score", "owner"):
        a, b = getattr(small, k), getattr(big, k)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert len(big.moves) == 7 and (big.moves >= 0).any(1).all()     # games were played, not only passes


# ---- 5. a board whose answer needs no network -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_engine", [True, False])
def test_the_board_that_needs_no_network(engine, with_engine):
    eng = engine if with_engine else None
    g = go.Game(BOARD)
    rec = records([g])
    assert T.area_score(torch.from_numpy(rec).to(DEV)).item() == 0.5
    fin = RO.finish_games(np.repeat(rec, 5, 0), eng, 17)
    assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 5 and fin.over.all() and fin.plies.tolist() == [3] * 5
    assert fin.score.tolist() == [3.5] * 5 and fin.unfinished == 0
    for n in (1, 8):
        r = RO.rollout_score([g], eng, n=n, seed=n)[0]
        assert r.score == 3.5 and r.black_win == 1.0 and r.mean_score == 3.5
        assert r.stones("dead") == [37] and r.stones("seki") == [] and len(r.stones("alive")) == 76
        assert r.mean_owner[37] == 1.0 and r.mean_owner[8] == -1.0 and r.unfinished == 0
    after = go.Game(BOARD)
    after.play_move(38)
    fin = RO.finish_games(records([after]), eng, 0)
    assert fin.moves.tolist() == [[go.PASS, go.PASS]] and fin.plies.tolist() == [2]
    assert fin.score[0] == T.area_score(torch.from_numpy(records([after])).to(DEV)).item() == 3.5
    both = RO.rollout_score([g, after], eng, n=4, seed=3)
    assert [b.score for b in both] == [3.5, 3.5] and both[1].stones("dead") == []


# ---- 6. the callers -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opponent():
    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    other = {k: (v + 0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(1), dtype=v.dtype)
                 if v.dtype.is_floating_point and "running_var" not in k else v) for k, v in sd.items()}
    e = R.policy_engine(other, 0, 512)
    yield e
    e.close()


def _host_area(recs):
    return np.array([go.golib().bk_pos_area_score(ctypes.cast(r.ctypes.data, _PP), 5.5) for r in recs], np.float32)


def test_play_games_finish(engine, opponent):
    W, B = 2, 24
    base = R.play_games(engine, opponent, W, B, seed=5, iteration=1, epoch=2)
    off = R.play_games(engine, opponent, W, B, seed=5, iteration=1, epoch=2, finish=False)
    on = R.play_games(engine, opponent, W, B, seed=5, iteration=1, epoch=2, finish=True)
    assert not hasattr(off, "finished") and not hasattr(base, "finished")
    for a in (off, on):
        assert np.array_equal(a.moves, base.moves) and np.array_equal(a.length, base.length)
        assert torch.equal(a.planes, base.planes) and torch.equal(a.played, base.played)
        assert torch.equal(a.logp.view(torch.int32), base.logp.view(torch.int32))
        assert np.array_equal(a.row_game, base.row_game) and np.array_equal(a.learner_black, base.learner_black)
    assert np.array_equal(off.black_wins, base.black_wins) and np.array_equal(off.reward, base.reward)
    # the rewards, recomputed on the host from the finished records (and from the board as it stands for a lagging game)
    fin, games = on.finished, on.finished_games
    assert len(games) > W * B // 2 and fin.unfinished == 0
    raw = R.initial_positions(W * B)
    for g in range(W * B):
        for mv in base.moves[g, :base.length[g]].tolist():
            assert R._play_fn()(raw[g].ctypes.data, mv) == 0
    score = _host_area(raw)
    assert np.array_equal(score > 0, base.black_wins)
    score[games] = _host_area(fin.records.cpu().numpy())
    assert np.array_equal(on.black_wins, score > 0)
    assert np.array_equal(on.reward, np.where((score > 0) == on.learner_black, 1.0, -1.0).astype(np.float32))
    # the finished records continue the games, colours kept: host rules give the same
    host = R.play_games(engine, opponent, W, B, seed=5, iteration=1, epoch=2, finish=True, rules="host")
    assert np.array_equal(host.finished_games, games)
    same = (host.finished.records == fin.records.cpu().numpy()).all(1)
    assert (~same).sum() <= MAX_DIFFERING_GAMES and (host.finished.min_margin[~same] < 1e-5).all()
    print(f"winner changed by finishing: {int((on.black_wins != base.black_wins).sum())}/{W * B}, "
          f"plies to the end mean {fin.plies.mean():.1f} max {fin.plies.max()}")


def test_generate_finish(engine, opponent):
    a = GV.generate(engine, opponent, 48, 48, seed=3)
    b = GV.generate(engine, opponent, 48, 48, seed=3, finish=True)
    assert np.array_equal(a.moves, b.moves) and np.array_equal(a.kept, b.kept) and np.array_equal(a.game, b.game)
    assert [r[:4] for r in a.rows] == [r[:4] for r in b.rows] and len(a.rows) > 40
    turn = np.array([r[3] for r in b.rows])
    assert [r[4] for r in b.rows] == np.where((turn % 2 == 0) == (b.score[b.game] > 0), 1, -1).tolist()
    h = GV.generate(engine, opponent, 48, 48, seed=3, finish=True, rules="host")
    assert (h.score != b.score).sum() <= MAX_DIFFERING_GAMES
    print(f"label changed by finishing: {sum(x[4] != y[4] for x, y in zip(a.rows, b.rows))}/{len(a.rows)}")


def test_gtp_rollout_score():
    from bokego_amd import nnet
    from bokego_amd.bkw import load_bkw
    from bokego_amd.gtp import NativeGTP
    from bokego_amd.mcts_native import Position
    pi = nnet.HipPolicyNet(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    val = nnet.HipValueNet(load_bkw(os.path.join(GOLDEN, "value_synth.bkw")))
    g = NativeGTP(Position(board=BOARD), pi, val, no_sim=True, time_lim=None, n_rollouts=10, rollout_score=8)
    g.running = True
    assert g.send("final_score") == "= B+3.5\n\n"
    assert g.send("final_status_list dead") == "= B5\n\n"
    assert g.send("final_status_list seki") == "= \n\n"
    assert g.send("play b c5") == "= \n\n" and g.send("final_score") == "= B+3.5\n\n"
    assert g.send("final_status_list dead") == "= \n\n"


def test_command_line_twice(tmp_path):
    """This test is about the command line: two runs with one seed print the same."""
    moves = json.load(open(os.path.join(GOLDEN, "playouts.json")))["moves"][0]
    sgf = str(tmp_path / "g.sgf")
    go.write_sgf(moves, sgf)
    cmd = [sys.executable, "-m", "bokego_amd.rollout", "--sgf", sgf, "--move", "20", "-p",
           os.path.join(GOLDEN, "policy_19.bkw"), "-n", "32", "--seed", "4"]
    outs = [subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=300) for _ in range(2)]
    assert outs[0].returncode == 0, outs[0].stderr[-2000:]
    assert outs[0].stdout == outs[1].stdout and outs[1].returncode == 0
    head = json.loads(outs[0].stdout.splitlines()[0])
    assert head["playouts"] == 32 and head["unfinished"] == 0 and 0.0 <= head["black_win"] <= 1.0
    assert len(outs[0].stdout.splitlines()) == 10

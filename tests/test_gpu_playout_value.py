"""-m gpu: bkt_random_playouts -- whole random playouts in one launch -- against its host mirror
(rollout.random_playouts(rules="host")), bit for bit; playout_value on the device against the host; and the callers
(PlayoutEvaluator, NativeMCTS(playout_value=), GTP --playout-value, self_play through both step loops)."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, nnet, selfplay
from bokego_amd import reinforce as R
from bokego_amd import rollout as RO
from bokego_amd.bkw import load_bkw
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_rollout_cpu import BOARD, records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NONE = RO.MOVE_NONE
CAP = 400


def _field(recs, off, dtype):
    return np.ascontiguousarray(recs[:, off:off + np.dtype(dtype).itemsize]).view(dtype)[:, 0]


def _golden_records():
    """positions.json: records built from boards (liberty cache invalid)."""
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


def _played_records(first=0, last=24):
    """playouts.json replayed with bk_pos_play alone: the liberty cache valid, a refresh pending at the last move."""
    games = json.load(open(os.path.join(GOLDEN, "playouts.json")))["moves"][first:last]
    play, out = R._play_fn(), []
    for moves in games:
        rec = R.initial_positions(1)
        for mv in moves:
            assert play(rec.ctypes.data, int(mv)) == 0
            out.append(rec[0].copy())
    return np.stack(out)


@pytest.fixture(scope="module")
def batch():
    """About 200 records: goldens with an invalid liberty cache, replayed records with a pending refresh, every kind with a
    ko set, and records whose last move is a pass.  200 = 66 full workgroups and a last one with two rows."""
    golden, played = _golden_records(), _played_records()
    both = np.concatenate([golden, played, _played_records(24, 256)])
    ko = both[_field(both, 164, np.int16) >= 0][:12]
    passed = np.concatenate([golden[5::40], played[3::60]])[:20].copy()
    for i in range(len(passed)):
        assert R._play_fn()(passed[i].ctypes.data, go.PASS) == 0
    n = (200 - len(ko) - len(passed)) // 2
    out = np.ascontiguousarray(np.concatenate([golden[::len(golden) // n][:n], played[::len(played) // n][:n], ko, passed]))
    assert 190 <= len(out) <= 200 and len(out) % 3 != 0
    assert (out[:, 162] == 0).sum() >= 60 and (out[:, 162] == 1).sum() >= 60          # cache invalid / valid
    assert (_field(out, 164, np.int16) >= 0).sum() >= 6 and (_field(out, 166, np.int16) == go.PASS).sum() >= 20
    return out


@pytest.fixture(scope="module")
def reference(batch):
    """(seed, the host mirror's games at the cap of 400): the first seed whose games hold one that two passes end before
    the cap -- chosen on the CPU, computed once."""
    for seed in range(8):
        host = RO.random_playouts(batch, seed, max_plies=CAP, rules="host")
        if (host.over & (host.plies < CAP)).any():
            return seed, host
    raise AssertionError("no seed in 0..7 ends a game before the cap")


def _assert_same(dev, host, what):
    got = dev.records.cpu().numpy()
    bad = np.nonzero((got != host.records).any(1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} records differ, first row {bad[0]} at bytes "
                           f"{np.nonzero(got[bad[0]] != host.records[bad[0]])[0][:8]}")
    assert np.array_equal(dev.plies, host.plies), (what, np.nonzero(dev.plies != host.plies)[0][:8])
    assert np.array_equal(dev.over, host.over), (what, np.nonzero(dev.over != host.over)[0][:8])
    assert dev.moves.shape == host.moves.shape and np.array_equal(dev.moves, host.moves), what
    assert dev.score.dtype == np.float32 and np.array_equal(dev.score.view(np.int32), host.score.view(np.int32)), what
    assert dev.owner.dtype == np.int8 and np.array_equal(dev.owner, host.owner), what
    assert dev.unfinished == host.unfinished


# ---- 1. the device equals the host mirror -----------------------------------------------------------------------------------
def test_whole_games_equal_the_host_mirror(batch, reference):
    seed, host = reference
    dev = RO.random_playouts(batch, seed, max_plies=CAP)
    print(f"seed {seed}: {len(batch)} games, plies mean {host.plies.mean():.1f} max {host.plies.max()}, "
          f"unfinished {host.unfinished}, black wins {int((host.score > 0).sum())}")
    _assert_same(dev, host, "cap 400")
    assert (host.over & (host.plies < CAP)).any()
    n = host.plies
    ended = np.nonzero(host.over)[0]
    assert all(dev.moves[g, n[g] - 1] == go.PASS and (dev.moves[g, n[g]:] == NONE).all() for g in ended.tolist())
    # from a device tensor, and again: the same bits; the caller's tensor is not played on
    t = torch.from_numpy(batch).to(DEV)
    again = RO.random_playouts(t, seed, max_plies=CAP)
    assert torch.equal(again.records, dev.records) and np.array_equal(again.moves, dev.moves)
    assert np.array_equal(t.cpu().numpy(), batch)


@pytest.mark.parametrize("max_plies", [1, 2])
def test_short_caps_equal_the_host_mirror(batch, reference, max_plies):
    seed = reference[0]
    host = RO.random_playouts(batch, seed, max_plies=max_plies, rules="host")
    dev = RO.random_playouts(batch, seed, max_plies=max_plies)
    _assert_same(dev, host, f"cap {max_plies}")
    assert dev.moves.shape == (len(batch), max_plies) and (dev.plies == max_plies).all()
    if max_plies == 1:
        assert dev.unfinished > 0 and not dev.over.all()             # the cap leaves rows unfinished
        # a record whose last move is a pass and that has no playable point ends with its first pass
        assert np.array_equal(dev.over, (dev.moves[:, 0] == go.PASS) & (_field(batch, 166, np.int16) == go.PASS))


@pytest.mark.parametrize("rows", [1, 3, 4, 7])
def test_small_batches_equal_the_host_mirror(batch, reference, rows):
    """A workgroup that is partial (1), full (3), full and a last one with one row (4, 7)."""
    seed = reference[0]
    part = batch[40:40 + rows]
    host = RO.random_playouts(part, seed, max_plies=CAP, rules="host")
    _assert_same(RO.random_playouts(part, seed, max_plies=CAP), host, f"{rows} rows")
    # with the counters of the big batch's rows: the big batch's games
    c = RO.default_counters(len(batch), RO.record_turns(batch))[40:40 + rows]
    sub = RO.random_playouts(part, seed, counters=c, max_plies=CAP)
    big = reference[1]
    assert np.array_equal(sub.records.cpu().numpy(), big.records[40:40 + rows])
    assert np.array_equal(sub.moves, big.moves[40:40 + rows, :sub.moves.shape[1]])


def test_the_largest_batch_equals_the_host_mirror(batch, reference):
    """T.MAX_BATCH rows, so that the row index inside the kernel runs up to 65,535 (the other tests stay below 600): row i
    holds record i % 200 with that record's counters and must play that record's game of the mirror, history included."""
    seed, big = reference
    n = len(batch)
    idx = torch.arange(T.MAX_BATCH, device=DEV) % n
    pos = torch.from_numpy(batch).to(DEV)[idx].contiguous()
    ctr = torch.from_numpy(RO.default_counters(n, RO.record_turns(batch))).to(DEV)[idx].contiguous()
    over, plies, moves, status = T.random_playouts(pos, seed, ctr, CAP)
    score, owner = T.area_score(pos, R.KOMI, owner=True)
    want_moves = np.full((n, CAP), NONE, np.int16)
    want_moves[:, :big.moves.shape[1]] = big.moves

    def rows(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)[idx]

    assert not status.any().item()
    assert torch.equal(pos, rows(big.records)) and torch.equal(moves, rows(want_moves))
    assert torch.equal(plies, rows(big.plies.astype(np.int32))) and torch.equal(over != 0, rows(big.over))
    assert torch.equal(score, rows(big.score)) and torch.equal(owner, rows(big.owner))


# ---- 2. rows that are over on entry ----------------------------------------------------------------------------------------------
def test_rows_over_on_entry_are_untouched(batch, reference):
    seed, big = reference
    recs = batch[:50]
    over = np.zeros(50, np.uint8)
    over[[0, 4, 5, 17, 30, 31, 32, 49]] = 1                          # a whole workgroup (30..32), and parts of others
    ctr = RO.default_counters(len(batch), RO.record_turns(batch))[:50]
    d = torch.from_numpy(recs).to(DEV)
    d_over = torch.from_numpy(over).to(DEV)
    got_over, plies, moves, status = T.random_playouts(d, seed, torch.from_numpy(ctr).to(DEV), CAP, over=d_over)
    assert got_over is d_over and not status.any().item()
    out, plies, moves = d.cpu().numpy(), plies.cpu().numpy(), moves.cpu().numpy()
    was = over != 0
    assert np.array_equal(out[was], recs[was]) and (plies[was] == 0).all() and (moves[was] == NONE).all()
    assert (d_over.cpu().numpy()[was] == 1).all()
    assert np.array_equal(out[~was], big.records[:50][~was]) and np.array_equal(plies[~was], big.plies[:50][~was])
    assert np.array_equal(d_over.cpu().numpy()[~was] != 0, big.over[:50][~was])
    L = big.moves.shape[1]
    assert np.array_equal(moves[~was][:, :L], big.moves[:50][~was]) and (moves[~was][:, L:] == NONE).all()


# ---- 3. the moves buffer and the argument checks ------------------------------------------------------------------------------
def test_without_a_history_and_bad_arguments(batch, reference):
    seed, big = reference
    quiet = RO.random_playouts(batch, seed, max_plies=CAP, history=False)
    assert quiet.moves is None
    assert np.array_equal(quiet.records.cpu().numpy(), big.records) and np.array_equal(quiet.score, big.score)
    assert np.array_equal(quiet.plies, big.plies) and np.array_equal(quiet.over, big.over)
    assert np.array_equal(quiet.owner, big.owner)

    lib = T.load()
    B = 5
    pos = torch.from_numpy(batch[:B].copy()).to(DEV)
    ctr = torch.from_numpy(RO.default_counters(B, np.zeros(B))).to(DEV)
    over = torch.zeros(B, dtype=torch.uint8, device=DEV)
    plies = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    status = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    moves = torch.full((B, 4), 7777, dtype=torch.int16, device=DEV)                  # no move: a move is in -2..80

    def call(p=pos.data_ptr(), batch_=B, c=ctr.data_ptr(), cap=4, o=over.data_ptr(), n=plies.data_ptr(), s=status.data_ptr()):
        return lib.bkt_random_playouts(p, batch_, seed, c, cap, o, n, moves.data_ptr(), s, None)

    for kw in (dict(batch_=0), dict(batch_=-1), dict(batch_=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025), dict(cap=-3),
               dict(p=None), dict(c=None), dict(o=None), dict(n=None), dict(s=None)):
        assert call(**kw) == -1, kw                                  # BKT_ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), batch[:B]) and not over.any().item()      # nothing was launched
    assert (plies == 77).all().item() and (status == 77).all().item() and (moves == 7777).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    m = moves.cpu().numpy()
    assert (plies.cpu().numpy() <= 4).all() and ((m >= NONE) & (m <= 80)).all()        # every entry is written
    assert RO.random_playouts(batch[:B], seed, max_plies=1024, history=False).unfinished == 0      # the largest cap
    with pytest.raises(ValueError, match="max_plies"):
        T.random_playouts(pos, seed, ctr, 1025)
    with pytest.raises(ValueError, match="max_plies"):
        RO.random_playouts(batch, seed, max_plies=0)


# ---- 4. playout_value ---------------------------------------------------------------------------------------------------------------
def test_playout_value_equals_the_host_and_belongs_to_the_record(batch):
    recs = batch[::8][:24]
    assert len(recs) == 24
    want = RO.playout_value(recs, 8, 21, rules="host")
    got = RO.playout_value(recs, 8, 21)
    assert got.dtype == np.float32 and got.shape == (24,)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.nonzero(got != want)[0]
    assert len(np.unique(want)) > 3                                  # the positions do differ
    others = batch[1::8][:24]
    rng = np.random.default_rng(3)
    perm = rng.permutation(24)
    mixed_idx = np.concatenate([perm, perm[:7], perm[::-1][:5]])     # shuffled, with duplicates
    mixed = np.empty((2 * len(mixed_idx), 192), np.uint8)
    mixed[0::2] = recs[mixed_idx]
    mixed[1::2] = others[rng.integers(0, 24, len(mixed_idx))]        # interleaved with other records
    v = RO.playout_value(torch.from_numpy(mixed).to(DEV), 8, 21)
    assert np.array_equal(v[0::2].view(np.int32), want[mixed_idx].view(np.int32))
    assert not np.array_equal(RO.playout_value(recs, 8, 22), got)    # the seed does enter


# ---- 5. the board whose value needs no luck, through the callers -----------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    net = nnet.HipPolicyNet(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    yield net


def test_the_board_through_the_callers(policy):
    g = go.Game(BOARD)
    after = go.Game(BOARD)
    after.play_move(38)
    rec = records([g, after])
    fin = RO.random_playouts(np.repeat(rec[:1], 4, 0), 2)
    assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 4 and fin.score.tolist() == [3.5] * 4 and fin.over.all()
    for n in (1, 8):
        assert RO.playout_value(rec, n, 5).tolist() == [1.0, -1.0]
        ev = RO.PlayoutEvaluator(policy.engine(), n, seed=5)
        probs, values = ev(rec, 1)
        assert probs.shape == (1, 81) and abs(float(probs.sum()) - 1) < 1e-5 and values.tolist() == [1.0, -1.0]
        assert values.dtype == np.float32 and (ev.positions, ev.batches) == (2, 1)
    r = RO.rollout_score([g], None, n=8, seed=1, one_launch=True)[0]
    assert r.score == 3.5 and r.black_win == 1.0 and r.stones("dead") == [37] and r.unfinished == 0
    # GTP: the launcher's flags, then the protocol on the same keywords
    args = gtp.parse_args(["--playout-value", "8", "-r", "16"])
    t = gtp.NativeGTP(Position(board=BOARD), policy, None, no_sim=not args.simulate, time_lim=None, n_rollouts=args.r,
                      rollout_score=args.rollout_score, playout_value=args.playout_value)
    assert isinstance(t.evaluator, RO.PlayoutEvaluator) and t.evaluator.playouts == 8 and t.evaluator.rules == "device"
    t.running = True
    t.rollout(4)
    assert t.root.value == 1.0
    assert t.send("genmove b") == "= C5\n\n"
    t.close()


# ---- 6. the tree search on the Monte-Carlo value --------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [250, 300])                        # middle-game boards: the host playouts of `b` stay short
def test_native_mcts_on_device_and_on_host_playouts(policy, index):
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][index]
    root = Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"])
    a = NativeMCTS(root, policy, None, playout_value=8, expand_thresh=4)
    b = NativeMCTS(root, evaluator=RO.PlayoutEvaluator(policy.engine(), 8, rules="host"), expand_thresh=4)
    assert isinstance(a.evaluator, RO.PlayoutEvaluator) and a.evaluator.rules == "device" and a.no_sim
    for t in (a, b):
        t.rollout(64)
    sa, sb = a.child_stats(), b.child_stats()
    assert sa == sb and sum(n for n, _ in sa.values()) >= 32 and len(sa) > 1
    assert a.winrate() == b.winrate() and 0.0 <= a.winrate() <= 1.0
    assert a.evaluator.positions == b.evaluator.positions and a.evaluator.batches == b.evaluator.batches
    assert a.choose().last_move == b.choose().last_move
    a.close()
    b.close()


# ---- 7. self-play through both step loops -------------------------------------------------------------------------------------------
def test_self_play_through_both_step_loops(policy):
    kw = dict(n_games=4, rollouts=16, expand_thresh=4, sample_plies=4, max_turns=12, cap=400, threads=2, n_pools=2)
    runs = []
    for native in (True, False, True):
        ev = RO.PlayoutEvaluator(policy.engine(), 4, seed=9)
        local, _ = selfplay.self_play(ev, native_loop=native, **kw)
        assert local["native_loop"] is native and ev.batches > 0 and ev.positions > 0
        runs.append({g: (v["moves"], v["score"]) for g, v in local["games"].items()})
    assert runs[0] == runs[1], "the C step loop and the Python step loop play different games"
    assert runs[0] == runs[2], "a second run with the same seeds plays other games"
    assert len(runs[0]) == 4 and all(len(m) > 0 for m, _ in runs[0].values())

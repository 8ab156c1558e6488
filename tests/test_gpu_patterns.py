"""-m gpu: the pattern-weighted playouts on the device -- bkt_pattern_codes against patterns.codes_host,
bkt_pattern_playouts against its host mirror (rollout.random_playouts(rules="host", patterns=)) bit for bit, constant tables
against bkt_random_playouts byte for byte, playout_value through a table, the fit's counts on the device against the host,
and the callers (NativeMCTS(playout_patterns=), self_play through both step loops)."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import go, nnet, selfplay
from bokego_amd import lockstep as L
from bokego_amd import patterns as PT
from bokego_amd import reinforce as R
from bokego_amd import rollout as RO
from bokego_amd.bkw import load_bkw
from bokego_amd.mcts_native import NativeMCTS, Position
from bokego_amd.train import load_weights
from conftest import GOLDEN
from test_rollout_cpu import BOARD, records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NONE = RO.MOVE_NONE
CAP = 400
SEED = 5


def _golden():
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


@pytest.fixture(scope="module")
def golden():
    return _golden()


@pytest.fixture(scope="module")
def table():
    """A seeded table over the whole uint16 range, zeros and 65535 included."""
    rng = np.random.default_rng(17)
    w = rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16)
    w[rng.integers(0, PT.ENTRIES, 4096)] = 0
    w[rng.integers(0, PT.ENTRIES, 4096)] = 65535
    w[0], w[1 << 16] = 0, 65535                                        # the empty pattern, far from and near the last move
    assert (w == 0).sum() > 3000 and (w == 65535).sum() > 3000
    return PT.PatternTable(w)


@pytest.fixture(scope="module")
def starts(golden):
    """64 games from the empty board and 8 mid-game goldens (both colours to move): 72 = 24 full workgroups."""
    mid = golden[60::len(golden) // 9][:8]
    assert len(mid) == 8 and len(set(L.black_to_move(mid).tolist())) == 2
    return np.ascontiguousarray(np.concatenate([R.initial_positions(64), mid]))


@pytest.fixture(scope="module")
def reference(starts, table):
    """The host mirror's games at the cap of 400, computed once."""
    return RO.random_playouts(starts, SEED, max_plies=CAP, rules="host", patterns=table)


def _assert_same(dev, host, what):
    got = dev.records.cpu().numpy()
    bad = np.nonzero((got != host.records).any(1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} records differ, first row {bad[0]} at bytes "
                           f"{np.nonzero(got[bad[0]] != host.records[bad[0]])[0][:8]}")
    assert np.array_equal(dev.plies, host.plies), (what, np.nonzero(dev.plies != host.plies)[0][:8])
    assert np.array_equal(dev.over, host.over), (what, np.nonzero(dev.over != host.over)[0][:8])
    assert dev.moves.shape == host.moves.shape and np.array_equal(dev.moves, host.moves), what
    assert dev.score.dtype == np.float32 and np.array_equal(dev.score.view(np.int32), host.score.view(np.int32)), what
    assert np.array_equal(dev.owner, host.owner), what
    assert dev.unfinished == host.unfinished


# ---- 1. the index ---------------------------------------------------------------------------------------------------------------
def test_codes_equal_the_host(golden):
    recs = golden[::7].copy()
    flipped = recs.copy()                                                # the same boards with the other colour to move
    flipped[:, 172] ^= 1
    passed = recs[:40].copy()
    passed[:, 166:168] = np.array([go.PASS], np.int16).view(np.uint8)    # the last move a pass
    none = recs[40:80].copy()
    none[:, 166:168] = np.array([-3], np.int16).view(np.uint8)           # no last move
    allrecs = np.ascontiguousarray(np.concatenate([recs, flipped, passed, none, R.initial_positions(1)]))
    want = PT.codes_host(allrecs)
    assert (want >= 1 << 16).any() and len(set(L.black_to_move(allrecs).tolist())) == 2
    before = torch.from_numpy(allrecs).to(DEV)
    got = T.pattern_codes(before)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(allrecs), 81)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(before.cpu().numpy(), allrecs)                 # the records are only read
    for rows in (1, 3, 4, 7):
        part = torch.from_numpy(allrecs[50:50 + rows]).to(DEV)
        assert np.array_equal(T.pattern_codes(part).cpu().numpy(), want[50:50 + rows]), rows
    lib = T.load()
    out = torch.full((3, 81), -7, dtype=torch.int32, device=DEV)
    for args in ((None, 3, out.data_ptr()), (before.data_ptr(), 3, None), (before.data_ptr(), 0, out.data_ptr()),
                 (before.data_ptr(), T.MAX_BATCH + 1, out.data_ptr())):
        assert lib.bkt_pattern_codes(*args, None) == -1
    torch.cuda.synchronize()
    assert (out == -7).all().item()


# ---- 2. whole games against the host mirror ---------------------------------------------------------------------------------
def test_whole_games_equal_the_host_mirror(starts, table, reference):
    dev = RO.random_playouts(starts, SEED, max_plies=CAP, patterns=table)
    print(f"{len(starts)} games, plies mean {reference.plies.mean():.1f} max {reference.plies.max()}, "
          f"unfinished {reference.unfinished}, black wins {int((reference.score > 0).sum())}")
    _assert_same(dev, reference, "cap 400")
    assert reference.over.sum() >= 64
    uniform = RO.random_playouts(starts, SEED, max_plies=CAP)
    assert not np.array_equal(uniform.moves[:, :10], dev.moves[:, :10])  # the table does enter
    t = torch.from_numpy(starts).to(DEV)
    again = RO.random_playouts(t, SEED, max_plies=CAP, patterns=table)
    assert torch.equal(again.records, dev.records) and np.array_equal(again.moves, dev.moves)
    assert np.array_equal(t.cpu().numpy(), starts)                       # the caller's tensor is not played on


@pytest.mark.parametrize("max_plies", [1, 2])
def test_short_caps_equal_the_host_mirror(starts, table, reference, max_plies):
    host = RO.random_playouts(starts, SEED, max_plies=max_plies, rules="host", patterns=table)
    dev = RO.random_playouts(starts, SEED, max_plies=max_plies, patterns=table)
    _assert_same(dev, host, f"cap {max_plies}")
    assert dev.moves.shape == (len(starts), max_plies) and (dev.plies == max_plies).all()
    assert np.array_equal(dev.moves, reference.moves[:, :max_plies])


@pytest.mark.parametrize("rows", [1, 3, 4, 7])
def test_small_batches_equal_the_host_mirror(starts, table, reference, rows):
    lo = 60                                                              # empty boards and mid-game records
    part = starts[lo:lo + rows]
    c = RO.default_counters(len(starts), RO.record_turns(starts))[lo:lo + rows]
    sub = RO.random_playouts(part, SEED, counters=c, max_plies=CAP, patterns=table)
    assert np.array_equal(sub.records.cpu().numpy(), reference.records[lo:lo + rows])
    width = sub.moves.shape[1]
    assert np.array_equal(sub.moves, reference.moves[lo:lo + rows, :width])
    assert (reference.moves[lo:lo + rows, width:] == NONE).all()
    assert np.array_equal(sub.plies, reference.plies[lo:lo + rows]) and np.array_equal(sub.over, reference.over[lo:lo + rows])
    assert np.array_equal(sub.score, reference.score[lo:lo + rows])


def test_rows_over_on_entry_without_a_history_and_bad_arguments(starts, table, reference):
    ctr = torch.from_numpy(RO.default_counters(len(starts), RO.record_turns(starts))).to(DEV)
    w = table.device(DEV)
    assert w.dtype == torch.int16 and table.device("cuda") is w          # the cached copy
    over = np.zeros(len(starts), np.uint8)
    over[[0, 4, 5, 17, 30, 31, 32, 66, 71]] = 1                          # a whole workgroup (30..32), and parts of others
    was = over != 0
    d = torch.from_numpy(starts).to(DEV)
    d_over = torch.from_numpy(over).to(DEV)
    got_over, plies, moves, status = T.pattern_playouts(d, SEED, ctr, w, CAP, over=d_over)
    assert got_over is d_over and not status.any().item()
    out, plies, moves = d.cpu().numpy(), plies.cpu().numpy(), moves.cpu().numpy()
    assert np.array_equal(out[was], starts[was]) and (plies[was] == 0).all() and (moves[was] == NONE).all()
    assert (d_over.cpu().numpy()[was] == 1).all()
    assert np.array_equal(out[~was], reference.records[~was]) and np.array_equal(plies[~was], reference.plies[~was])
    width = reference.moves.shape[1]
    assert np.array_equal(moves[~was][:, :width], reference.moves[~was]) and (moves[~was][:, width:] == NONE).all()
    # moves = NULL
    quiet = RO.random_playouts(starts, SEED, max_plies=CAP, history=False, patterns=table)
    assert quiet.moves is None and np.array_equal(quiet.records.cpu().numpy(), reference.records)
    assert np.array_equal(quiet.plies, reference.plies) and np.array_equal(quiet.score, reference.score)
    # the bad arguments: BKT_ERR_ARG and nothing launched
    lib = T.load()
    B = 5
    pos = torch.from_numpy(starts[62:62 + B].copy()).to(DEV)
    c5 = ctr[62:62 + B].contiguous()
    ov = torch.zeros(B, dtype=torch.uint8, device=DEV)
    n = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    st = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    mv = torch.full((B, 4), 7777, dtype=torch.int16, device=DEV)

    def call(p=pos.data_ptr(), batch_=B, c=c5.data_ptr(), t=w.data_ptr(), cap=4, o=ov.data_ptr(), n_=n.data_ptr(),
             s=st.data_ptr()):
        return lib.bkt_pattern_playouts(p, batch_, SEED, c, t, cap, o, n_, mv.data_ptr(), s, None)

    for kw in (dict(batch_=0), dict(batch_=-1), dict(batch_=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025), dict(cap=-3),
               dict(p=None), dict(c=None), dict(t=None), dict(o=None), dict(n_=None), dict(s=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), starts[62:62 + B]) and not ov.any().item()
    assert (n == 77).all().item() and (st == 77).all().item() and (mv == 7777).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(mv.cpu().numpy(), reference.moves[62:62 + B, :4])
    assert np.array_equal(n.cpu().numpy(), np.minimum(reference.plies[62:62 + B], 4))
    with pytest.raises(ValueError, match="max_plies"):
        T.pattern_playouts(pos, SEED, c5, w, 1025)
    with pytest.raises(ValueError):
        T.pattern_playouts(pos, SEED, c5, w[:100].contiguous(), 4)
    with pytest.raises(ValueError):
        T.pattern_playouts(pos, SEED, c5, torch.from_numpy(table.array.view(np.int16).copy()), 4)     # a table on the host


# ---- 3. the identity: a constant table plays bkt_random_playouts' games --------------------------------------------------------
@pytest.mark.parametrize("c", [65535, 1])
def test_a_constant_table_is_the_uniform_kernel(c):
    start = R.initial_positions(64)
    ctr = torch.from_numpy(RO.default_counters(64, RO.record_turns(start))).to(DEV)
    a, b = torch.from_numpy(start).to(DEV), torch.from_numpy(start).to(DEV)
    assert 81 * c == (5308335 if c == 65535 else 81)                     # S at the first ply: the 64-bit product
    over_a, plies_a, moves_a, status_a = T.random_playouts(a, SEED, ctr, CAP)
    over_b, plies_b, moves_b, status_b = T.pattern_playouts(b, SEED, ctr, PT.PatternTable.constant(c).device(DEV), CAP)
    assert torch.equal(a, b) and torch.equal(moves_a, moves_b) and torch.equal(plies_a, plies_b)
    assert torch.equal(over_a, over_b) and not status_b.any().item() and over_b.all().item()
    assert not np.array_equal(a.cpu().numpy(), start)


# ---- 4. the value ---------------------------------------------------------------------------------------------------------------
def test_playout_value_equals_the_host_and_belongs_to_the_record(golden, table):
    recs = golden[30::25][:12]
    assert len(recs) == 12
    want = RO.playout_value(recs, 8, 21, rules="host", patterns=table)
    got = RO.playout_value(recs, 8, 21, patterns=table)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), np.nonzero(got != want)[0]
    assert len(np.unique(want)) > 2
    rng = np.random.default_rng(3)
    perm = rng.permutation(12)
    idx = np.concatenate([perm, perm[:5], perm[::-1][:4]])               # shuffled, with duplicates
    v = RO.playout_value(torch.from_numpy(np.ascontiguousarray(recs[idx])).to(DEV), 8, 21, patterns=table)
    assert np.array_equal(v.view(np.int32), want[idx].view(np.int32))
    assert not np.array_equal(RO.playout_value(recs, 8, 21), got)        # not the uniform playouts' value
    same = RO.playout_value(recs, 8, 21, patterns=PT.PatternTable.constant(3))
    assert np.array_equal(same, RO.playout_value(recs, 8, 21))


def test_the_board_that_needs_no_luck(table):
    rec = records([go.Game(BOARD)])
    for t in (table, PT.PatternTable.constant(0), PT.PatternTable.constant(65535)):
        fin = RO.random_playouts(np.repeat(rec, 4, 0), 2, patterns=t)
        assert fin.moves.tolist() == [[38, go.PASS, go.PASS]] * 4 and fin.score.tolist() == [3.5] * 4 and fin.over.all()
    assert RO.playout_value(rec, 8, 5, patterns=table).tolist() == [1.0]
    r = RO.rollout_score([go.Game(BOARD)], None, n=8, seed=1, one_launch=True, patterns=table)[0]
    assert r.score == 3.5 and r.black_win == 1.0 and r.stones("dead") == [37]


# ---- 5. the fit -----------------------------------------------------------------------------------------------------------------
def test_counts_on_the_device_equal_the_host():
    eng = R.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 8)
    try:
        start = R.initial_positions(8)
        fin = RO.finish_games(start, eng, 3)
    finally:
        eng.close()
    assert fin.over.all() and fin.moves.shape[1] > 40
    want = PT.counts(start, fin.moves, rules="host")
    got = PT.counts(start, fin.moves)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1].sum() == (fin.moves >= 0).sum()                        # finish_games' moves are all playable
    assert got[0].sum() > 20 * got[1].sum()
    # from a tensor on the device, and the table the fit makes of it
    again = PT.counts(torch.from_numpy(start).to(DEV), fin.moves)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    fitted = PT.fit(start, fin.moves)
    assert np.array_equal(fitted.array, PT.weights(*PT.symmetrise(*want)))
    assert fitted.array[0] == PT.weights(*PT.symmetrise(*want))[0] and len(np.unique(fitted.array)) > 10


# ---- 6. the callers -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    net = nnet.HipPolicyNet(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    yield net


@pytest.mark.parametrize("index", [250, 300])
def test_native_mcts_on_device_and_on_host_playouts(policy, table, index):
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][index]
    root = Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"])
    a = NativeMCTS(root, policy, None, playout_value=16, playout_patterns=table, expand_thresh=4)
    b = NativeMCTS(root, evaluator=RO.PlayoutEvaluator(policy.engine(), 16, rules="host", patterns=table), expand_thresh=4)
    assert isinstance(a.evaluator, RO.PlayoutEvaluator) and a.evaluator.rules == "device" and a.evaluator.patterns is table
    for t in (a, b):
        t.rollout(32)
    sa, sb = a.child_stats(), b.child_stats()
    assert sa == sb and sum(n for n, _ in sa.values()) >= 16 and len(sa) > 1
    assert a.winrate() == b.winrate() and 0.0 <= a.winrate() <= 1.0
    assert a.evaluator.positions == b.evaluator.positions and a.evaluator.batches == b.evaluator.batches
    assert a.choose().last_move == b.choose().last_move
    a.close()
    b.close()


def test_self_play_through_both_step_loops(policy, table):
    kw = dict(n_games=2, rollouts=8, expand_thresh=4, sample_plies=2, max_turns=6, cap=400, threads=2, n_pools=1)
    runs = []
    for native, rules in ((True, "device"), (False, "device"), (True, "host")):
        ev = RO.PlayoutEvaluator(policy.engine(), 4, seed=9, rules=rules, patterns=table)
        local, _ = selfplay.self_play(ev, native_loop=native, **kw)
        assert local["native_loop"] is native and ev.batches > 0 and ev.positions > 0
        runs.append({g: (v["moves"], v["score"]) for g, v in local["games"].items()})
    assert runs[0] == runs[1], "the C step loop and the Python step loop play different games"
    assert runs[0] == runs[2], "the device playouts and the host playouts play different games"
    assert len(runs[0]) == 2 and all(len(m) > 0 for m, _ in runs[0].values())
    plain = RO.PlayoutEvaluator(policy.engine(), 4, seed=9)
    assert plain.patterns is None

"""-m gpu: the tactical playouts on the device -- bkt_tactical_codes against tactics.codes_host,
bkt_tactical_playouts against its host mirror (rollout.random_playouts(rules="host", tactics=)) bit for bit with and without
a pattern table, neutral tactics against bkt_pattern_playouts and bkt_random_playouts byte for byte, playout_value through
the tables, the fit's counts on the device against the host, and the callers (NativeMCTS(playout_tactics=), self_play
through both step loops).  The inputs are test_gpu_patterns.py's."""
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
from bokego_amd import tactics as TC
from bokego_amd.bkw import load_bkw
from bokego_amd.mcts_native import NativeMCTS, Position
from bokego_amd.train import load_weights
from conftest import GOLDEN
from test_gpu_patterns import _assert_same, _golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NONE = RO.MOVE_NONE
CAP = 400
SEED = 5


@pytest.fixture(scope="module")
def golden():
    return _golden()


@pytest.fixture(scope="module")
def table():
    """test_gpu_patterns.py's seeded pattern table over the whole uint16 range."""
    rng = np.random.default_rng(17)
    w = rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16)
    w[rng.integers(0, PT.ENTRIES, 4096)] = 0
    w[rng.integers(0, PT.ENTRIES, 4096)] = 65535
    w[0], w[1 << 16] = 0, 65535
    return PT.PatternTable(w)


@pytest.fixture(scope="module")
def tactics():
    """A seeded tactics table over the whole uint16 range, 0 and 65535 present on codes that occur."""
    rng = np.random.default_rng(23)
    t = rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16)
    t[8], t[4], t[9], t[20] = 65535, 0, 65535, 0        # a quiet point, a point with two liberties, a capture, an escape
    assert (t == 0).sum() >= 2 and (t == 65535).sum() >= 2
    return TC.TacticTable(t)


@pytest.fixture(scope="module")
def starts(golden):
    """64 games from the empty board and 8 mid-game goldens (both colours to move): 72 = 24 full workgroups."""
    mid = golden[60::len(golden) // 9][:8]
    assert len(mid) == 8 and len(set(L.black_to_move(mid).tolist())) == 2
    return np.ascontiguousarray(np.concatenate([R.initial_positions(64), mid]))


@pytest.fixture(scope="module")
def references(starts, table, tactics):
    """The host mirror's games at the cap of 400, with and without the pattern table, computed once."""
    return {True: RO.random_playouts(starts, SEED, max_plies=CAP, rules="host", patterns=table, tactics=tactics),
            False: RO.random_playouts(starts, SEED, max_plies=CAP, rules="host", tactics=tactics)}


def _patterns(table, with_table):
    return table if with_table else None


# ---- 1. the code ----------------------------------------------------------------------------------------------------------------
def test_codes_equal_the_host(golden):
    recs = golden[::7].copy()
    flipped = recs.copy()                                                # the same boards with the other colour to move
    flipped[:, 172] ^= 1
    passed = recs[:40].copy()
    passed[:, 166:168] = np.array([go.PASS], np.int16).view(np.uint8)    # the last move a pass
    none = recs[40:80].copy()
    none[:, 166:168] = np.array([-3], np.int16).view(np.uint8)           # no last move
    allrecs = np.ascontiguousarray(np.concatenate([recs, flipped, passed, none, R.initial_positions(1)]))
    want = TC.codes_host(allrecs)
    assert ((want & 3) > 0).any() and ((want >> 4) & 1).any() and ((want >> 5) & 1).any()
    assert want.min() >= 0 and want.max() < TC.ENTRIES and len(set(L.black_to_move(allrecs).tolist())) == 2
    before = torch.from_numpy(allrecs).to(DEV)
    got = T.tactical_codes(before)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(allrecs), 81)
    bad = np.nonzero((got.cpu().numpy() != want).any(1))[0]
    assert len(bad) == 0, (bad[:8], got.cpu().numpy()[bad[0]], want[bad[0]])
    assert np.array_equal(before.cpu().numpy(), allrecs)                 # the records are only read
    for rows in (1, 3, 4, 7):
        part = torch.from_numpy(allrecs[50:50 + rows]).to(DEV)
        assert np.array_equal(T.tactical_codes(part).cpu().numpy(), want[50:50 + rows]), rows
    lib = T.load()
    out = torch.full((3, 81), -7, dtype=torch.int32, device=DEV)
    for args in ((None, 3, out.data_ptr()), (before.data_ptr(), 3, None), (before.data_ptr(), 0, out.data_ptr()),
                 (before.data_ptr(), T.MAX_BATCH + 1, out.data_ptr())):
        assert lib.bkt_tactical_codes(*args, None) == -1
    torch.cuda.synchronize()
    assert (out == -7).all().item()


# ---- 2. whole games against the host mirror ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_table", [True, False])
def test_whole_games_equal_the_host_mirror(starts, table, tactics, references, with_table):
    ref, pat = references[with_table], _patterns(table, with_table)
    dev = RO.random_playouts(starts, SEED, max_plies=CAP, patterns=pat, tactics=tactics)
    print(f"{len(starts)} games, plies mean {ref.plies.mean():.1f} max {ref.plies.max()}, unfinished {ref.unfinished}, "
          f"black wins {int((ref.score > 0).sum())}")
    _assert_same(dev, ref, f"cap 400, patterns {with_table}")
    assert ref.over.sum() >= 48
    plain = RO.random_playouts(starts, SEED, max_plies=CAP, patterns=pat)
    assert not np.array_equal(plain.moves[:, :10], dev.moves[:, :10])    # the tactics do enter
    t = torch.from_numpy(starts).to(DEV)
    again = RO.random_playouts(t, SEED, max_plies=CAP, patterns=pat, tactics=tactics)
    assert torch.equal(again.records, dev.records) and np.array_equal(again.moves, dev.moves)
    assert np.array_equal(t.cpu().numpy(), starts)                       # the caller's tensor is not played on


@pytest.mark.parametrize("with_table", [True, False])
@pytest.mark.parametrize("max_plies", [1, 2])
def test_short_caps_equal_the_host_mirror(starts, table, tactics, references, max_plies, with_table):
    pat = _patterns(table, with_table)
    host = RO.random_playouts(starts, SEED, max_plies=max_plies, rules="host", patterns=pat, tactics=tactics)
    dev = RO.random_playouts(starts, SEED, max_plies=max_plies, patterns=pat, tactics=tactics)
    _assert_same(dev, host, f"cap {max_plies}")
    assert dev.moves.shape == (len(starts), max_plies) and (dev.plies == max_plies).all()
    assert np.array_equal(dev.moves, references[with_table].moves[:, :max_plies])


@pytest.mark.parametrize("with_table", [True, False])
@pytest.mark.parametrize("rows", [1, 3, 4, 7])
def test_small_batches_equal_the_host_mirror(starts, table, tactics, references, rows, with_table):
    ref = references[with_table]
    lo = 60                                                              # empty boards and mid-game records
    part = starts[lo:lo + rows]
    c = RO.default_counters(len(starts), RO.record_turns(starts))[lo:lo + rows]
    sub = RO.random_playouts(part, SEED, counters=c, max_plies=CAP, patterns=_patterns(table, with_table), tactics=tactics)
    assert np.array_equal(sub.records.cpu().numpy(), ref.records[lo:lo + rows])
    width = sub.moves.shape[1]
    assert np.array_equal(sub.moves, ref.moves[lo:lo + rows, :width])
    assert (ref.moves[lo:lo + rows, width:] == NONE).all()
    assert np.array_equal(sub.plies, ref.plies[lo:lo + rows]) and np.array_equal(sub.over, ref.over[lo:lo + rows])
    assert np.array_equal(sub.score, ref.score[lo:lo + rows]) and np.array_equal(sub.owner, ref.owner[lo:lo + rows])


def test_rows_over_on_entry_without_a_history_and_bad_arguments(starts, table, tactics, references):
    reference = references[True]
    ctr = torch.from_numpy(RO.default_counters(len(starts), RO.record_turns(starts))).to(DEV)
    w, tw = table.device(DEV), tactics.device(DEV)
    assert tw.dtype == torch.int16 and tactics.device("cuda") is tw      # the cached copy
    over = np.zeros(len(starts), np.uint8)
    over[[0, 4, 5, 17, 30, 31, 32, 66, 71]] = 1                          # a whole workgroup (30..32), and parts of others
    was = over != 0
    d = torch.from_numpy(starts).to(DEV)
    d_over = torch.from_numpy(over).to(DEV)
    got_over, plies, moves, status = T.tactical_playouts(d, SEED, ctr, w, tw, CAP, over=d_over)
    assert got_over is d_over and not status.any().item()
    out, plies, moves = d.cpu().numpy(), plies.cpu().numpy(), moves.cpu().numpy()
    assert np.array_equal(out[was], starts[was]) and (plies[was] == 0).all() and (moves[was] == NONE).all()
    assert (d_over.cpu().numpy()[was] == 1).all()
    assert np.array_equal(out[~was], reference.records[~was]) and np.array_equal(plies[~was], reference.plies[~was])
    width = reference.moves.shape[1]
    assert np.array_equal(moves[~was][:, :width], reference.moves[~was]) and (moves[~was][:, width:] == NONE).all()
    # moves = NULL
    for with_table in (True, False):
        ref = references[with_table]
        quiet = RO.random_playouts(starts, SEED, max_plies=CAP, history=False, patterns=_patterns(table, with_table),
                                   tactics=tactics)
        assert quiet.moves is None and np.array_equal(quiet.records.cpu().numpy(), ref.records)
        assert np.array_equal(quiet.plies, ref.plies) and np.array_equal(quiet.score, ref.score)
    # the bad arguments: BKT_ERR_ARG and nothing launched; a NULL pattern table is no bad argument
    lib = T.load()
    B = 5
    pos = torch.from_numpy(starts[62:62 + B].copy()).to(DEV)
    c5 = ctr[62:62 + B].contiguous()
    ov = torch.zeros(B, dtype=torch.uint8, device=DEV)
    n = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    st = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    mv = torch.full((B, 4), 7777, dtype=torch.int16, device=DEV)

    def call(p=pos.data_ptr(), batch_=B, c=c5.data_ptr(), t=w.data_ptr(), tt=tw.data_ptr(), cap=4, o=ov.data_ptr(),
             n_=n.data_ptr(), s=st.data_ptr()):
        return lib.bkt_tactical_playouts(p, batch_, SEED, c, t, tt, cap, o, n_, mv.data_ptr(), s, None)

    for kw in (dict(batch_=0), dict(batch_=-1), dict(batch_=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025), dict(cap=-3),
               dict(p=None), dict(c=None), dict(tt=None), dict(o=None), dict(n_=None), dict(s=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), starts[62:62 + B]) and not ov.any().item()
    assert (n == 77).all().item() and (st == 77).all().item() and (mv == 7777).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(mv.cpu().numpy(), reference.moves[62:62 + B, :4])
    assert np.array_equal(n.cpu().numpy(), np.minimum(reference.plies[62:62 + B], 4))
    pos.copy_(torch.from_numpy(starts[62:62 + B]))
    ov.zero_()
    assert call(t=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(mv.cpu().numpy(), references[False].moves[62:62 + B, :4])
    with pytest.raises(ValueError, match="max_plies"):
        T.tactical_playouts(pos, SEED, c5, w, tw, 1025)
    with pytest.raises(ValueError):
        T.tactical_playouts(pos, SEED, c5, w, tw[:10].contiguous(), 4)
    with pytest.raises(ValueError):
        T.tactical_playouts(pos, SEED, c5, w[:100].contiguous(), tw, 4)
    with pytest.raises(ValueError):
        T.tactical_playouts(pos, SEED, c5, w, torch.from_numpy(tactics.array.view(np.int16).copy()), 4)   # on the host


# ---- 3. the identities: neutral tactics play the siblings' games ------------------------------------------------------------------
def test_neutral_tactics_are_the_pattern_kernel(starts, table):
    ctr = torch.from_numpy(RO.default_counters(len(starts), RO.record_turns(starts))).to(DEV)
    a, b = torch.from_numpy(starts).to(DEV), torch.from_numpy(starts).to(DEV)
    over_a, plies_a, moves_a, status_a = T.pattern_playouts(a, SEED, ctr, table.device(DEV), CAP)
    over_b, plies_b, moves_b, status_b = T.tactical_playouts(b, SEED, ctr, table.device(DEV),
                                                             TC.TacticTable.neutral().device(DEV), CAP)
    assert torch.equal(a, b) and torch.equal(moves_a, moves_b) and torch.equal(plies_a, plies_b)
    assert torch.equal(over_a, over_b) and torch.equal(status_a, status_b) and not status_b.any().item()
    assert not np.array_equal(a.cpu().numpy(), starts)


def test_neutral_tactics_without_a_table_are_the_uniform_kernel(starts):
    ctr = torch.from_numpy(RO.default_counters(len(starts), RO.record_turns(starts))).to(DEV)
    a, b = torch.from_numpy(starts).to(DEV), torch.from_numpy(starts).to(DEV)
    over_a, plies_a, moves_a, status_a = T.random_playouts(a, SEED, ctr, CAP)
    over_b, plies_b, moves_b, status_b = T.tactical_playouts(b, SEED, ctr, None, TC.TacticTable.neutral().device(DEV), CAP)
    assert torch.equal(a, b) and torch.equal(moves_a, moves_b) and torch.equal(plies_a, plies_b)
    assert torch.equal(over_a, over_b) and torch.equal(status_a, status_b) and not status_b.any().item()
    assert not np.array_equal(a.cpu().numpy(), starts)


# ---- 4. the value ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_table", [True, False])
def test_playout_value_equals_the_host_and_belongs_to_the_record(golden, table, tactics, with_table):
    pat = _patterns(table, with_table)
    recs = golden[30::25][:12]
    assert len(recs) == 12
    want = RO.playout_value(recs, 8, 21, rules="host", patterns=pat, tactics=tactics)
    got = RO.playout_value(recs, 8, 21, patterns=pat, tactics=tactics)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), np.nonzero(got != want)[0]
    assert len(np.unique(want)) > 2
    rng = np.random.default_rng(3)
    perm = rng.permutation(12)
    idx = np.concatenate([perm, perm[:5], perm[::-1][:4]])               # shuffled, with duplicates
    v = RO.playout_value(torch.from_numpy(np.ascontiguousarray(recs[idx])).to(DEV), 8, 21, patterns=pat, tactics=tactics)
    assert np.array_equal(v.view(np.int32), want[idx].view(np.int32))
    assert not np.array_equal(RO.playout_value(recs, 8, 21, patterns=pat), got)      # the tactics enter the value
    same = RO.playout_value(recs, 8, 21, patterns=pat, tactics=TC.TacticTable.neutral())
    assert np.array_equal(same, RO.playout_value(recs, 8, 21, patterns=pat))


# ---- 5. the fit -----------------------------------------------------------------------------------------------------------------
def test_counts_on_the_device_equal_the_host(table):
    eng = R.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 8)
    try:
        start = R.initial_positions(8)
        fin = RO.finish_games(start, eng, 3)
    finally:
        eng.close()
    assert fin.over.all() and fin.moves.shape[1] > 40
    for pat in (None, table):
        mass_h, played_h = TC.counts(start, fin.moves, pat, rules="host")
        mass_d, played_d = TC.counts(start, fin.moves, pat)
        assert played_d.dtype == np.int64 and mass_d.dtype == np.float64 and mass_d.shape == (TC.ENTRIES,)
        assert np.array_equal(played_d, played_h)
        assert played_d.sum() == (fin.moves >= 0).sum()                  # finish_games' moves are all playable
        err = np.abs(mass_d - mass_h) / np.maximum(np.abs(mass_h), 1e-300)
        print("mass: largest relative difference", err[mass_h > 0].max())
        assert ((mass_h > 0) == (mass_d > 0)).all() and (err[mass_h > 0] <= 1e-8).all()
        # the expected plays of all codes together: one per ply that had a playable point
        assert abs(mass_h.sum() - played_h.sum()) < 1e-6 and (played_h[[c for c in range(64) if c & 3]].sum() > 0)
    again = TC.counts(torch.from_numpy(start).to(DEV), fin.moves, table)
    assert np.array_equal(again[1], played_h)
    fitted = TC.fit(start, fin.moves, table)
    assert isinstance(fitted, TC.TacticTable) and len(np.unique(fitted.array)) > 5


# ---- 6. the callers -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    net = nnet.HipPolicyNet(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    yield net


@pytest.mark.parametrize("index", [250, 300])
def test_native_mcts_on_device_and_on_host_playouts(policy, table, tactics, index):
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][index]
    root = Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"])
    a = NativeMCTS(root, policy, None, playout_value=16, playout_patterns=table, playout_tactics=tactics, expand_thresh=4)
    b = NativeMCTS(root, evaluator=RO.PlayoutEvaluator(policy.engine(), 16, rules="host", patterns=table, tactics=tactics),
                   expand_thresh=4)
    assert isinstance(a.evaluator, RO.PlayoutEvaluator) and a.evaluator.rules == "device"
    assert a.evaluator.patterns is table and a.evaluator.tactics is tactics
    for t in (a, b):
        t.rollout(32)
    sa, sb = a.child_stats(), b.child_stats()
    assert sa == sb and sum(n for n, _ in sa.values()) >= 16 and len(sa) > 1
    assert a.winrate() == b.winrate() and 0.0 <= a.winrate() <= 1.0
    assert a.evaluator.positions == b.evaluator.positions and a.evaluator.batches == b.evaluator.batches
    assert a.choose().last_move == b.choose().last_move
    a.close()
    b.close()


def test_self_play_through_both_step_loops(policy, table, tactics):
    kw = dict(n_games=2, rollouts=8, expand_thresh=4, sample_plies=2, max_turns=6, cap=400, threads=2, n_pools=1)
    runs = []
    for native, rules in ((True, "device"), (False, "device"), (True, "host")):
        ev = RO.PlayoutEvaluator(policy.engine(), 4, seed=9, rules=rules, patterns=table, tactics=tactics)
        local, _ = selfplay.self_play(ev, native_loop=native, **kw)
        assert local["native_loop"] is native and ev.batches > 0 and ev.positions > 0
        runs.append({g: (v["moves"], v["score"]) for g, v in local["games"].items()})
    assert runs[0] == runs[1], "the C step loop and the Python step loop play different games"
    assert runs[0] == runs[2], "the device playouts and the host playouts play different games"
    assert len(runs[0]) == 2 and all(len(m) > 0 for m, _ in runs[0].values())
    plain = RO.PlayoutEvaluator(policy.engine(), 4, seed=9)
    assert plain.patterns is None and plain.tactics is None

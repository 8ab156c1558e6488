"""-m gpu: the move weights of a position in one launch on the MI355X (bkt_move_weights, rollout.move_weights),
integer for integer against the host mirror, against the composition of the three launches it replaces, and against the
first moves of the tactical playouts; the argument checks; and the evaluator and the tree search on a prior with the
pattern term, device rules against host rules."""
import ctypes

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import reinforce as R
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from test_amaf_cpu import seeded_tables, three_records
from test_pattern_prior_cpu import (SEED, check_first_moves, eyes_only_record, first_moves, golden_records, ko_record,
                                    played_records)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BATCHES = (1, 2, 3, 4, 7, 130)     # one seat; a tail workgroup with two and with one idle seat; a full one plus one record; many
SENTINEL = 0x5A5A5A5A
COMBOS = ((False, False), (True, False), (False, True), (True, True))


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def pool():
    """130 records.  The first nine: test_gpu_amaf.py's five (the board that needs no luck, the empty board, a record after
    a pass, two mid-game goldens, one per colour), the empty board, a record after a pass, a ko, and a full board with only
    eye points left.  Then goldens from all over the games (liberty cache invalid) and replayed playouts (cache valid, a
    refresh pending at the last move)."""
    gold = golden_records()
    black = L.black_to_move(gold)
    mid = np.stack([gold[60], gold[61 + int(np.argmax(black[61:] != black[60]))]])
    three = three_records()
    played = played_records(3)
    recs = np.concatenate([three, mid, R.initial_positions(1), three[2:3], ko_record(), eyes_only_record(),
                           gold[::len(gold) // 60][:60], played[np.linspace(5, len(played) - 1, 61).astype(int)]])
    assert len(recs) == 130 and (recs[:, 162] == 0).sum() > 60 and (recs[:, 162] == 1).sum() > 60
    return np.ascontiguousarray(recs)


@pytest.fixture(scope="module")
def mirror(pool, tables):
    """The host mirror of the whole pool for the four table combinations, computed once."""
    return {c: RO.move_weights_host(pool, tables[0] if c[0] else None, tables[1] if c[1] else None) for c in COMBOS}


def _tables(tables, combo):
    return tables[0] if combo[0] else None, tables[1] if combo[1] else None


def _device(recs, pat, tac):
    d = torch.from_numpy(np.ascontiguousarray(recs)).to(DEV)
    w = T.move_weights(d, None if pat is None else pat.device(DEV), None if tac is None else tac.device(DEV))
    assert w.dtype == torch.int32 and tuple(w.shape) == (len(recs), 81) and w.device == d.device
    assert np.array_equal(d.cpu().numpy(), recs)                      # the records are read only
    return w.cpu().numpy()


@pytest.mark.parametrize("batch", BATCHES)
def test_device_equals_the_mirror(pool, tables, mirror, batch):
    for combo in COMBOS:
        got = _device(pool[:batch], *_tables(tables, combo))
        want = mirror[combo][:batch]
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (combo, f"{len(bad)} rows differ, first {bad[0]} at points {np.nonzero(got[bad[0]] != want[bad[0]])[0]}")
    if batch >= 9:
        assert not mirror[(True, True)][8].any() and mirror[(True, True)][7, 10] == 0      # eyes only; the ko point
        assert np.array_equal(mirror[(False, False)][:batch], 256 * RO.playable_host(pool[:batch]))
    # records that are somewhere else in the batch give the same row: nothing depends on the seat
    if batch == 7:
        got = _device(pool[:7][::-1], *tables)
        assert np.array_equal(got[::-1], mirror[(True, True)][:7])
    # the public call, from numpy records and from records that are on the device already
    assert np.array_equal(RO.move_weights(pool[:batch], *tables), mirror[(True, True)][:batch])
    assert np.array_equal(RO.move_weights(torch.from_numpy(pool[:batch]).to(DEV), tables[0]), mirror[(True, False)][:batch])


@pytest.mark.parametrize("batch", BATCHES)
def test_device_equals_the_composition_of_three_launches(pool, tables, batch):
    recs = pool[:batch]
    d = torch.from_numpy(recs).to(DEV)
    idx = T.pattern_codes(d).to(torch.int64)
    code = T.tactical_codes(d).to(torch.int64)
    scratch = d.clone()
    playable = torch.empty((batch, 81), dtype=torch.uint8, device=DEV)
    status = T.playout_step(scratch, torch.full((batch,), T.MOVE_NONE, dtype=torch.int32, device=DEV), None, None, playable)
    assert not status.any() and torch.equal(scratch, d)
    for combo in COMBOS:
        pat, tac = _tables(tables, combo)
        P = torch.full((batch, 81), 256, dtype=torch.int64, device=DEV)
        Tw = torch.full((batch, 81), 256, dtype=torch.int64, device=DEV)
        if pat is not None:
            P = (pat.device(DEV).to(torch.int64) & 0xFFFF)[idx].clamp_(min=1)
        if tac is not None:
            Tw = (tac.device(DEV).to(torch.int64) & 0xFFFF)[code]
        want = ((P * Tw) >> 8).clamp_(min=1) * (playable != 0)
        got = T.move_weights(d, None if pat is None else pat.device(DEV), None if tac is None else tac.device(DEV))
        assert torch.equal(got.to(torch.int64), want), combo


def test_weights_give_the_first_moves_of_the_tactical_playouts(pool, tables):
    recs = pool[:9]
    pat, tac = tables
    for p in (pat, None):
        w = _device(recs, p, tac)
        d = torch.from_numpy(np.repeat(recs, 7, 0)).to(DEV)
        ctr = torch.from_numpy(RO.default_counters(len(d), RO.record_turns(np.repeat(recs, 7, 0)))).to(DEV)
        _, plies, moves, status = T.tactical_playouts(d, SEED, ctr, None if p is None else p.device(DEV), tac.device(DEV), 1,
                                                      history=True)
        assert not status.any() and moves.shape == (63, 1)
        x0 = L.philox4x32_10(ctr.cpu().numpy().view(np.uint32), L.seed_key(L.seed_u64(SEED)))[:, 0].reshape(9, 7)
        check_first_moves(w, moves.cpu().numpy()[:, 0].reshape(9, 7), x0)
        host_moves, host_x0 = first_moves(recs, p, tac, rules="device")   # the public path draws with the same words
        assert np.array_equal(host_x0, x0) and np.array_equal(host_moves, moves.cpu().numpy()[:, 0].reshape(9, 7))


def test_output_is_fully_overwritten_and_bad_arguments_leave_it(pool, tables, mirror):
    lib = T.load()
    pat, tac = (t.device(DEV) for t in tables)
    s = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for batch in (1, 4, 130):
        d = torch.from_numpy(pool[:batch]).to(DEV)
        out = torch.full((batch + 1, 81), SENTINEL, dtype=torch.int32, device=DEV)
        assert lib.bkt_move_weights(d.data_ptr(), batch, pat.data_ptr(), tac.data_ptr(), out.data_ptr(), s) == 0
        got = out.cpu().numpy()
        assert (got[batch] == SENTINEL).all()                          # nothing past the batch
        assert np.array_equal(got[:batch], mirror[(True, True)][:batch]) and (got[:batch] < 1 << 24).all()
    d = torch.from_numpy(pool[:4]).to(DEV)
    out = torch.full((4, 81), SENTINEL, dtype=torch.int32, device=DEV)
    for args in ((None, 4, pat.data_ptr(), tac.data_ptr(), out.data_ptr()),
                 (d.data_ptr(), 4, pat.data_ptr(), tac.data_ptr(), None),
                 (d.data_ptr(), 0, pat.data_ptr(), tac.data_ptr(), out.data_ptr()),
                 (d.data_ptr(), -1, None, None, out.data_ptr()),
                 (d.data_ptr(), T.MAX_BATCH + 1, None, None, out.data_ptr())):
        assert lib.bkt_move_weights(*args, s) == -1, args[1]
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and np.array_equal(d.cpu().numpy(), pool[:4])
    # the binding refuses what tactical_codes refuses, and tables of the wrong length, dtype or device
    for bad in (d[:, :100], d[:0], d.cpu(), d.to(torch.int8)):
        with pytest.raises(ValueError):
            T.tactical_codes(bad)
        with pytest.raises(ValueError):
            T.move_weights(bad)
    for kw in (dict(table=pat[:100]), dict(table=pat.to(torch.int32)), dict(table=pat.cpu()), dict(tactics=tac[:63]),
               dict(tactics=tac.to(torch.float32)), dict(tactics=tac.cpu()), dict(table=tables[0].array)):
        with pytest.raises(ValueError):
            T.move_weights(d, **kw)


def test_the_evaluator_with_a_pattern_prior_equals_the_host_rules(pool, tables):
    pat, tac = tables
    recs = np.ascontiguousarray(pool[[0, 3, 4, 7, 1]])
    for rave in (False, True):
        dev, host = (RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1, pattern_prior=1, prior_patterns=pat, prior_tactics=tac,
                                         rave=rave, rules=rules) for rules in ("device", "host"))
        out_d, out_h = dev(recs, 3), host(recs, 3)
        assert len(out_d) == len(out_h) == 2 + rave
        assert out_d[0].shape == (3, 81) and np.array_equal(out_d[0].view(np.int32), out_h[0].view(np.int32))
        assert np.array_equal(out_d[1].view(np.int32), out_h[1].view(np.int32))
        plain = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1, rave=rave)(recs, 3)
        assert np.array_equal(plain[1], out_d[1]) and not np.array_equal(plain[0][1], out_d[0][1])
        if rave:
            for d, h, p in zip(out_d[2][1:], out_h[2][1:], plain[2][1:]):
                assert np.array_equal(d, h) and np.array_equal(d, p)
    from bokego_amd.selfplay import normalise_like_categorical
    want = normalise_like_categorical(RO.amaf_prior(recs[:3], RO.playout_amaf(recs[:3], 8, SEED),
                                                    weights=RO.move_weights(recs[:3], pat, tac), mu=1.0))
    assert np.array_equal(out_d[0].view(np.int32), want.view(np.int32))
    # the playouts' own tables, with criticality on top
    dev, host = (RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1, pattern_prior=0.5, patterns=pat, tactics=tac, criticality=1.0,
                                     rules=rules) for rules in ("device", "host"))
    out_d, out_h = dev(recs, 2), host(recs, 2)
    assert np.array_equal(out_d[0].view(np.int32), out_h[0].view(np.int32)) and np.array_equal(out_d[1], out_h[1])


def test_native_mcts_with_a_pattern_prior_device_against_host_rules(tables):
    """A late middle game (58 stones), so that the host rules' playouts are short: 60 rollouts, net-free, RAVE on."""
    import json
    import os

    from conftest import GOLDEN
    r = max(json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"], key=lambda r: sum(c != "." for c in r["board"]))
    seen = []
    for rules in ("device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=8, playout_prior=1, playout_pattern_prior=1, playout_rave=4, prior_patterns=tables[0],
                       prior_tactics=tables[1], expand_thresh=3, playout_seed=SEED, playout_rules=rules)
        assert t.evaluator.rules == rules and t.evaluator.rave and t.evaluator.pattern_prior == 1.0
        t.rollout(60)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move))
        t.close()
    assert seen[0] == seen[1]
    assert sum(seen[0][0].values()) == 60 and seen[0][1] in seen[0][0]

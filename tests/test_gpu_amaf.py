"""-m gpu: the AMAF counts on the MI355X (bkt_amaf_counts, rollout.playout_amaf) against the host mirror, integer
for integer and bit for bit: hand-written histories, whole playouts with and without tables, the argument checks, and the
evaluator, self-play and the tree search on a prior that needs no network."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import go, selfplay
from bokego_amd import lockstep as L
from bokego_amd import reinforce as R
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import (BOARD, HAND_MOVES, HAND_PLAYED, HAND_WON, HAND_WON_AT, KW, NONE, PASS, seeded_tables,
                           three_records)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
FIELDS = ("value", "wins", "played", "won")


def _golden():
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


@pytest.fixture(scope="module")
def five():
    """The board that needs no luck, the empty board, a record after a pass, and two mid-game goldens, one per colour."""
    gold = _golden()
    black = L.black_to_move(gold)
    mid = np.stack([gold[60], gold[61 + int(np.argmax(black[61:] != black[60]))]])
    recs = np.ascontiguousarray(np.concatenate([three_records(), mid]))
    assert len(recs) == 5 and len(set(L.black_to_move(mid).tolist())) == 2 and (mid[:, :81] != 0).sum(1).min() > 10
    return recs


@pytest.fixture(scope="module")
def many():
    """130 records: more workgroups than 128, with an odd tail; two empty boards and goldens from all over the games."""
    gold = _golden()
    return np.ascontiguousarray(np.concatenate([R.initial_positions(2), gold[::len(gold) // 128][:128]]))


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


def _same(dev, host, what):
    for f in FIELDS:
        d, h = getattr(dev, f), getattr(host, f)
        assert d.dtype == h.dtype and d.shape == h.shape, (what, f)
        assert np.array_equal(d.view(np.int32), h.view(np.int32)), (what, f, np.nonzero(d != h)[0][:8])
    assert dev.n == host.n


def _counts(moves, won, records, playouts):
    played, won_at = T.amaf_counts(torch.from_numpy(np.ascontiguousarray(moves)).to(DEV),
                                   torch.from_numpy(np.ascontiguousarray(won, np.uint8)).to(DEV), records, playouts)
    assert played.dtype == won_at.dtype == torch.int32 and played.shape == won_at.shape == (records, 81)
    return played.cpu().numpy(), won_at.cpu().numpy()


# ---- 8. hand-written histories -------------------------------------------------------------------------------------------------
def test_counts_equal_the_hand_written_ones():
    played, won_at = _counts(HAND_MOVES, HAND_WON, 2, 3)
    assert np.array_equal(played, HAND_PLAYED) and np.array_equal(won_at, HAND_WON_AT)
    host = RO.amaf_counts_host(HAND_MOVES, HAND_WON, 2, 3)
    assert np.array_equal(played, host[0]) and np.array_equal(won_at, host[1])
    played, won_at = _counts(HAND_MOVES, HAND_WON, 6, 1)              # one playout a record: three idle waves
    host = RO.amaf_counts_host(HAND_MOVES, HAND_WON, 6, 1)
    assert np.array_equal(played, host[0]) and np.array_equal(won_at, host[1])


def test_the_longest_rows_and_the_shortest():
    # max_plies = 1024, five playouts (two rounds of a workgroup, the second with one row).  Row 0: passes, and the only move
    # that counts at ply 1022, behind every staging stride; the opponent's answer at 1023 does not count.  Row 1: a move at
    # ply 1023 alone.  Row 2: over from the start.  Row 3: the same point at 1022, lost.  Row 4: its end marker at ply 1021.
    moves = np.full((5, 1024), PASS, np.int16)
    moves[0, 1022], moves[0, 1023] = 33, 34
    moves[1, 1023] = 35
    moves[2] = NONE
    moves[3, 1022] = 33
    moves[4, 1021], moves[4, 1022] = NONE, 36
    won = np.array([1, 1, 1, 0, 1], np.uint8)
    want_played, want_won = np.zeros((1, 81), np.int32), np.zeros((1, 81), np.int32)
    want_played[0, 33], want_won[0, 33] = 2, 1
    played, won_at = _counts(moves, won, 1, 5)
    assert np.array_equal(played, want_played) and np.array_equal(won_at, want_won)
    host = RO.amaf_counts_host(moves, won, 1, 5)
    assert np.array_equal(host[0], want_played) and np.array_equal(host[1], want_won)
    # records = playouts = max_plies = 1
    for entry, w, n in ((7, 1, 1), (7, 0, 1), (PASS, 1, 0), (NONE, 1, 0), (81, 1, 0), (80, 1, 1)):
        played, won_at = _counts(np.array([[entry]], np.int16), [w], 1, 1)
        assert played.sum() == n and won_at.sum() == n * w and (n == 0 or played[0, entry] == 1), entry
    with pytest.raises(ValueError):
        T.amaf_counts(torch.zeros((6, 8), dtype=torch.int16, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV), 2, 4)
    with pytest.raises(ValueError):
        T.amaf_counts(torch.zeros((6, 8), dtype=torch.int32, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV), 2, 3)
    with pytest.raises(ValueError):
        T.amaf_counts(torch.zeros((6, 8), dtype=torch.int16, device=DEV), torch.zeros(6, dtype=torch.uint8), 2, 3)
    with pytest.raises(ValueError):
        T.amaf_counts(torch.zeros((6, 1025), dtype=torch.int16, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV), 2, 3)


@pytest.mark.parametrize("records,playouts,max_plies", [(3, 9, 37), (7, 4, 401), (2, 6, 3)])
def test_any_history_gives_the_mirrors_counts(records, playouts, max_plies):
    """Entries of every kind, the ones no playout writes included (above 80, below the end marker), at widths that are no
    multiple of the four entries a read takes: wrong histories give the mirror's counts, and nothing is indexed by them."""
    rng = np.random.default_rng(records * 1000 + max_plies)
    moves = rng.integers(-1, 81, (records * playouts, max_plies)).astype(np.int16)
    odd = rng.random(moves.shape)
    moves[odd < 0.03] = rng.choice(np.array([81, 82, 127, 128, 255, 256, 32767, -3, -4, -32768], np.int16), int((odd < 0.03).sum()))
    moves[rng.random(moves.shape) < 0.01] = NONE
    won = rng.integers(0, 2, records * playouts).astype(np.uint8)
    played, won_at = _counts(moves, won, records, playouts)
    host = RO.amaf_counts_host(moves, won, records, playouts)
    assert np.array_equal(played, host[0]) and np.array_equal(won_at, host[1]) and played.sum() > 0


# ---- 9, 10. whole playouts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_tables", [False, True])
def test_playouts_equal_the_host_mirror_and_the_value(five, tables, with_tables):
    kw = dict(patterns=tables[0]) if with_tables else {}
    host = RO.playout_amaf(five, 7, SEED, rules="host", **kw)
    dev = RO.playout_amaf(five, 7, SEED, rules="device", **kw)
    _same(dev, host, with_tables)
    assert dev.played[0].tolist() == [7 if s == 38 else 0 for s in range(81)] and dev.wins[0] == 7
    assert dev.played[1:3].sum(1).min() > 7 * 5 and dev.played[3:].sum(1).min() > 0 and (dev.won <= dev.played).all() and (dev.played <= 7).all()
    value = RO.playout_value(five, 7, SEED, rules="device", **kw)
    assert value.dtype == np.float32 and np.array_equal(dev.value.view(np.int32), value.view(np.int32))
    on_device = RO.playout_amaf(torch.from_numpy(five).to(DEV), 7, SEED, **kw)      # records that are there already
    _same(on_device, host, with_tables)
    if with_tables:                                                   # and with the tactical weights on top
        kw["tactics"] = tables[1]
        both = RO.playout_amaf(five, 7, SEED, **kw)
        _same(both, RO.playout_amaf(five, 7, SEED, rules="host", **kw), "tactics")
        assert np.array_equal(both.value.view(np.int32), RO.playout_value(five, 7, SEED, **kw).view(np.int32))
        assert not np.array_equal(both.played, dev.played)


def test_one_playout_of_many_records(many):
    host = RO.playout_amaf(many, 1, SEED, rules="host")
    dev = RO.playout_amaf(many, 1, SEED, rules="device")
    _same(dev, host, "130 x 1")
    assert np.array_equal(dev.value.view(np.int32), RO.playout_value(many, 1, SEED).view(np.int32))
    assert (dev.played <= 1).all() and dev.played[:2].sum(1).min() > 5 and np.array_equal(dev.played[0], dev.played[1])


# ---- 11. the argument checks -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    lib = T.load()
    moves = torch.from_numpy(HAND_MOVES).to(DEV)
    won = torch.from_numpy(HAND_WON).to(DEV)
    played = torch.full((2, 81), 77, dtype=torch.int32, device=DEV)
    won_at = torch.full((2, 81), 77, dtype=torch.int32, device=DEV)

    def call(m=moves.data_ptr(), cap=8, w=won.data_ptr(), records=2, playouts=3, p=played.data_ptr(), wa=won_at.data_ptr()):
        return lib.bkt_amaf_counts(m, cap, w, records, playouts, p, wa, None)

    for kw in (dict(m=None), dict(w=None), dict(p=None), dict(wa=None), dict(records=0), dict(records=-2), dict(playouts=0),
               dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30),
               dict(cap=0), dict(cap=-8), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (played == 77).all().item() and (won_at == 77).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(played.cpu().numpy(), HAND_PLAYED) and np.array_equal(won_at.cpu().numpy(), HAND_WON_AT)


# ---- 12. the evaluator, self-play and the tree ----------------------------------------------------------------------------------
def test_the_net_free_evaluator_equals_the_host_rules(five):
    recs = np.ascontiguousarray(np.concatenate([five, five[1:2]]))
    dev, host = (RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rules=rules) for rules in ("device", "host"))
    (p_dev, v_dev), (p_host, v_host) = dev(recs, 2), host(recs, 2)
    assert p_dev.shape == (2, 81) and v_dev.shape == (6,) and p_dev.dtype == v_dev.dtype == np.float32
    assert np.array_equal(p_dev.view(np.int32), p_host.view(np.int32)) and np.array_equal(v_dev.view(np.int32), v_host.view(np.int32))
    assert np.array_equal(v_dev, RO.playout_value(recs, 8, SEED)) and v_dev[1] == v_dev[5]
    p, v = dev(recs, 0)
    assert p.shape == (0, 81) and np.array_equal(v, v_dev)
    games = []
    for rules in ("device", "host"):
        ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rules=rules)
        local, _ = selfplay.self_play(ev, native_loop=True, **dict(KW, max_turns=4))
        assert ev.batches > 0
        games.append(local["games"])
    assert games[0] == games[1] and len(games[0]) == 2


def test_native_mcts_without_a_network():
    t = NativeMCTS(Position(), None, None, playout_value=8, playout_prior=1.0, playout_seed=SEED)
    assert t.evaluator.policy_engine is None and t.evaluator.rules == "device"
    t.rollout(20)
    child = t.choose()
    assert 0 <= child.last_move < 81
    t.close()
    t = NativeMCTS(Position(board=BOARD), None, None, playout_value=8, playout_prior=1.0, expand_thresh=1)
    t.rollout(6)
    assert t.root.value == 1.0 and t.choose().last_move == 38
    t.close()

"""-m gpu: the two-sided AMAF counts on the MI355X (bkt_amaf_counts_sides) against the host mirror and against
bkt_amaf_counts, integer for integer; the argument checks; playout_amaf(sides=2), the RAVE evaluator and the net-free tree
search with RAVE, device rules against host rules."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import go
from bokego_amd import lockstep as L
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import HAND_MOVES, HAND_PLAYED, HAND_WON, HAND_WON_AT, NONE, PASS, seeded_tables, three_records
from test_rave_cpu import HAND_PLAYED_1, HAND_WON_AT_1

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5


def _golden():
    return json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]


def _record(r):
    return np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"])._pos), np.uint8)


@pytest.fixture(scope="module")
def five():
    """test_gpu_amaf's five: the board that needs no luck, the empty board, a record after a pass, and two mid-game goldens,
    one per colour."""
    gold = np.stack([_record(r) for r in _golden()])
    black = L.black_to_move(gold)
    mid = np.stack([gold[60], gold[61 + int(np.argmax(black[61:] != black[60]))]])
    return np.ascontiguousarray(np.concatenate([three_records(), mid]))


def _history(records, playouts, max_plies):
    """HAND_MOVES at its own shape; else entries of every kind, the ones no playout writes included (above 80, below the end
    marker), as test_gpu_amaf's test_any_history_gives_the_mirrors_counts draws them."""
    if (records, playouts, max_plies) == (2, 3, 8):
        return HAND_MOVES, HAND_WON
    rng = np.random.default_rng(records * 1000 + max_plies)
    moves = rng.integers(-1, 81, (records * playouts, max_plies)).astype(np.int16)
    odd = rng.random(moves.shape)
    moves[odd < 0.03] = rng.choice(np.array([81, 82, 127, 128, 255, 256, 32767, -3, -4, -32768], np.int16), int((odd < 0.03).sum()))
    moves[rng.random(moves.shape) < 0.01] = NONE
    if max_plies == 1024:                                                 # the longest row: a first play at its last ply
        moves[0, :] = PASS
        moves[0, 1023] = 33
    return moves, rng.integers(0, 2, records * playouts).astype(np.uint8) * np.uint8(201)


# (1,1,1): one row, one entry; (2,3,8): the hand-written histories; (3,9,37): three rounds, the last with one row; (7,4,401) and
# (2,6,3): widths that are no multiple of four, one full round and a tail round with two idle waves; (1,5,1024): the longest row;
# (130,1,8): more workgroups than 128, three idle waves each
@pytest.mark.parametrize("records,playouts,max_plies", [(1, 1, 1), (2, 3, 8), (3, 9, 37), (7, 4, 401), (2, 6, 3), (1, 5, 1024),
                                                         (130, 1, 8)])
def test_the_device_equals_the_mirror_and_side_0_the_one_sided_kernel(records, playouts, max_plies):
    moves, won = _history(records, playouts, max_plies)
    m, w = torch.from_numpy(np.ascontiguousarray(moves)).to(DEV), torch.from_numpy(np.ascontiguousarray(won)).to(DEV)
    played, won_at = T.amaf_counts_sides(m, w, records, playouts)
    assert played.dtype == won_at.dtype == torch.int32 and played.shape == won_at.shape == (records, 2, 81)
    one = T.amaf_counts(m, w, records, playouts)
    played, won_at = played.cpu().numpy(), won_at.cpu().numpy()
    host = RO.amaf_counts_sides_host(moves, won, records, playouts)
    assert np.array_equal(played, host[0]), np.argwhere(played != host[0])[:8]
    assert np.array_equal(won_at, host[1]), np.argwhere(won_at != host[1])[:8]
    assert np.array_equal(played[:, 0], one[0].cpu().numpy()) and np.array_equal(won_at[:, 0], one[1].cpu().numpy())
    assert (played.sum(1) <= playouts).all() and (won_at <= played).all() and (won_at >= 0).all()
    if max_plies == 8 and records == 2:
        assert np.array_equal(played[:, 0], HAND_PLAYED) and np.array_equal(won_at[:, 0], HAND_WON_AT)
        assert np.array_equal(played[:, 1], HAND_PLAYED_1) and np.array_equal(won_at[:, 1], HAND_WON_AT_1)
    elif max_plies > 1:
        assert played[:, 0].sum() > 0 and played[:, 1].sum() > 0
    if max_plies == 1024:
        assert played[0, 1, 33] >= 1                                      # ply 1023 is the opponent's


def test_bad_arguments_are_refused_and_nothing_is_written():
    lib = T.load()
    moves = torch.from_numpy(HAND_MOVES).to(DEV)
    won = torch.from_numpy(HAND_WON).to(DEV)
    played = torch.full((2, 2, 81), 77, dtype=torch.int32, device=DEV)
    won_at = torch.full((2, 2, 81), 77, dtype=torch.int32, device=DEV)

    def call(m=moves.data_ptr(), cap=8, w=won.data_ptr(), records=2, playouts=3, p=played.data_ptr(), wa=won_at.data_ptr()):
        return lib.bkt_amaf_counts_sides(m, cap, w, records, playouts, p, wa, None)

    for kw in (dict(m=None), dict(w=None), dict(p=None), dict(wa=None), dict(records=0), dict(records=-2), dict(playouts=0),
               dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30),
               dict(cap=0), dict(cap=-8), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (played == 77).all().item() and (won_at == 77).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(played.cpu().numpy()[:, 1], HAND_PLAYED_1) and np.array_equal(won_at.cpu().numpy()[:, 1], HAND_WON_AT_1)
    for bad in ((torch.zeros((6, 8), dtype=torch.int16, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV), 2, 4),
                (torch.zeros((6, 8), dtype=torch.int32, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV), 2, 3),
                (torch.zeros((6, 8), dtype=torch.int16, device=DEV), torch.zeros(6, dtype=torch.uint8), 2, 3),
                (torch.zeros((6, 1025), dtype=torch.int16, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV), 2, 3)):
        with pytest.raises(ValueError):
            T.amaf_counts_sides(*bad)


@pytest.mark.parametrize("with_tables", [False, True])
def test_playout_amaf_with_both_sides_equals_the_host_mirror(five, with_tables):
    kw = dict(zip(("patterns", "tactics"), seeded_tables())) if with_tables else {}
    host = RO.playout_amaf(five, 7, SEED, rules="host", sides=2, **kw)
    dev = RO.playout_amaf(five, 7, SEED, rules="device", sides=2, **kw)
    for f in ("value", "wins", "played", "won"):
        d, h = getattr(dev, f), getattr(host, f)
        assert d.dtype == h.dtype and d.shape == h.shape and np.array_equal(d.view(np.int32), h.view(np.int32)), f
    assert dev.played.shape == (5, 2, 81) and (dev.played.sum(1) <= 7).all() and dev.played[1:, 1].sum(1).min() > 0
    one = RO.playout_amaf(five, 7, SEED, rules="device", **kw)            # sides=1: the one-sided kernel, the same integers
    assert np.array_equal(one.played, dev.played[:, 0]) and np.array_equal(one.won, dev.won[:, 0])
    assert np.array_equal(one.value.view(np.int32), dev.value.view(np.int32)) and np.array_equal(one.wins, dev.wins)


def test_the_rave_evaluator_equals_the_host_rules(five):
    recs = np.ascontiguousarray(np.concatenate([five, five[1:2]]))
    dev, host = (RO.PlayoutEvaluator(None, 7, seed=SEED, prior=1.0, rave=True, rules=rules) for rules in ("device", "host"))
    (p_dev, v_dev, r_dev), (p_host, v_host, r_host) = dev(recs, 2), host(recs, 2)
    assert p_dev.shape == (2, 81) and v_dev.shape == (6,) and p_dev.dtype == v_dev.dtype == np.float32
    assert np.array_equal(p_dev.view(np.int32), p_host.view(np.int32)) and np.array_equal(v_dev.view(np.int32), v_host.view(np.int32))
    assert r_dev[0] == r_host[0] == 7
    for d, h, shape in zip(r_dev[1:], r_host[1:], ((6,), (6, 2, 81), (6, 2, 81))):
        assert d.dtype == h.dtype == np.int32 and d.shape == h.shape == shape and np.array_equal(d, h)
    plain = RO.PlayoutEvaluator(None, 7, seed=SEED, prior=1.0)(recs, 2)  # probs and values as without RAVE
    assert len(plain) == 2 and np.array_equal(plain[0], p_dev) and np.array_equal(plain[1], v_dev)
    assert np.array_equal(r_dev[2][1], r_dev[2][5]) and np.array_equal(v_dev, ((2 * r_dev[1] - 7) / np.float32(7)).astype(np.float32))


def test_native_mcts_with_rave_device_against_host_rules():
    """A late middle game (58 stones), so that the host rules' playouts are short: 60 rollouts, net-free, RAVE on."""
    r = max(_golden(), key=lambda r: sum(c != "." for c in r["board"]))
    seen = []
    for rules in ("device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=8, playout_prior=1.0, playout_rave=16, expand_thresh=3, playout_seed=SEED, playout_rules=rules)
        assert t.evaluator.rules == rules and t.evaluator.rave
        t.rollout(60)
        rn, rw = t.rave()
        stats = {mv: n for mv, (n, _) in t.child_stats().items()}
        seen.append((stats, rn.tolist(), rw.tolist(), t.choose().last_move))
        t.close()
    assert seen[0] == seen[1]
    stats, rn, rw, move = seen[0]
    assert sum(stats.values()) == 60 and sum(rn) > 60 * 8 and all(0 <= b <= a for a, b in zip(rn, rw)) and move in stats

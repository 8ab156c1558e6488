"""-m gpu: ownership and criticality on the MI355X (bkt_owner_counts, rollout.playout_ownership) against the host
mirror and against bkt_area_score's owner array reduced in numpy, integer for integer and bit for bit: every shape of a
round, boards of one colour and of nobody, the argument checks, whole playouts with and without tables, the evaluator and
the net-free tree search with the criticality term, and the GTP engine that scores its games by its own playouts."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp
from bokego_amd import lockstep as L
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import seeded_tables, three_records
from test_ownership_cpu import COUNTS, DEAD, HAND, hand_records, reduced, same_counts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
KOMI = 5.5


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


def _special():
    """An all-black board (margin 81), an all-white one (-81), and a board of dame only: no stone, nobody's region."""
    empty = np.frombuffer(bytes(go.Game()._pos), np.uint8)
    out = np.stack([empty, empty, empty]).copy()
    out[0, :81], out[1, :81] = 1, 2
    return out


@pytest.fixture(scope="module")
def boards(five):
    """The final boards the shapes below are cut from (numpy uint8 [643,192]): the three special boards, the final records
    of 64 device playouts of each of the five in a seeded order, and the same 320 in their own order -- and what the mirror
    and bkt_area_score say of every row, once."""
    fin = RO.random_playouts(np.repeat(five, 64, 0), SEED, history=False, device=DEV).records.cpu().numpy()
    final = np.ascontiguousarray(np.concatenate([_special(), fin[np.random.default_rng(3).permutation(320)], fin]))
    score, owner = T.area_score(torch.from_numpy(final).to(DEV), KOMI, owner=True)
    return final, owner.cpu().numpy(), score.cpu().numpy(), RO.owner_host(final)


def _device_counts(rows, records, playouts, komi=KOMI):
    pos = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    before = pos.clone()
    out = T.owner_counts(pos, records, playouts, komi)
    for x, shape in zip(out, ((records, 81),) * 3 + ((records, 163), (records,))):
        assert x.dtype == torch.int32 and tuple(x.shape) == shape and x.device == pos.device
    assert torch.equal(pos, before)                                       # the records are read only
    return tuple(x.cpu().numpy() for x in out)


# ---- 1. device against mirror ----------------------------------------------------------------------------------------------------
def test_the_hand_example():
    same_counts(_device_counts(hand_records(), 1, 3), HAND)
    same_counts(_device_counts(hand_records(), 1, 3), RO.owner_counts_host(hand_records(), 1, 3, KOMI))
    same_counts(_device_counts(hand_records(), 3, 1), RO.owner_counts_host(hand_records(), 3, 1, KOMI))
    same_counts(_device_counts(hand_records(), 1, 3, -0.5), RO.owner_counts_host(hand_records(), 1, 3, -0.5))


# (1,1): one board, two idle seats; (1,2) and (2,4): tail rounds with two idle seats and with one; (3,7): three rounds, the
# last with one board; (5,64): 22 rounds, the last with one; (130,1): more workgroups than 128, two idle seats each
@pytest.mark.parametrize("records,playouts", [(1, 1), (1, 2), (2, 4), (3, 7), (5, 64), (130, 1)])
def test_counts_equal_the_mirror_and_the_reduced_owner_array(boards, records, playouts):
    final, owner, score, owner_h = boards
    assert np.array_equal(owner, owner_h)
    G = records * playouts
    sl = slice(0, G) if G < 320 else slice(323, 323 + G)                 # (5,64): the playouts of each of the five, in order
    rows = final[sl]
    got = _device_counts(rows, records, playouts)
    same_counts(got, RO.owner_counts_host(rows, records, playouts, KOMI))
    same_counts(got, reduced(owner[sl], score[sl] > 0, records, playouts))
    assert got[3].sum(1).tolist() == [playouts] * records and (got[0] + got[1] <= playouts).all()
    if G >= 3 and G < 320:                                                # the special boards lead
        r1, r2 = 1 // playouts, 2 // playouts
        assert got[3][0, 162] >= 1 and got[3][r1, 0] >= 1 and got[3][r2, 81] >= 1
    if (records, playouts) == (5, 64):
        assert got[4][0] == 64 and got[3][0, 81 + 9] == 64 and 0 < got[4][1] < 64      # no luck needed; the empty board
        assert np.abs(RO.criticality_of(got[0], got[1], got[2], got[4], 64)[1:]).max() > 0.05


def test_boards_of_one_colour_and_of_nobody():
    b, w, a, h, bw = _device_counts(_special(), 3, 1)
    assert (b[0] == 1).all() and not w[0].any() and (a[0] == 1).all() and h[0, 162] == 1 and h[0].sum() == 1 and bw[0] == 1
    assert (w[1] == 1).all() and not b[1].any() and (a[1] == 1).all() and h[1, 0] == 1 and h[1].sum() == 1 and bw[1] == 0
    assert not b[2].any() and not w[2].any() and not a[2].any() and h[2, 81] == 1 and h[2].sum() == 1 and bw[2] == 0
    same_counts((b, w, a, h, bw), RO.owner_counts_host(_special(), 3, 1, KOMI))
    same_counts(_device_counts(_special(), 1, 3, -0.5), RO.owner_counts_host(_special(), 1, 3, -0.5))   # dame wins at komi < 0
    assert _device_counts(_special(), 1, 3, -0.5)[4].tolist() == [2]


# ---- 2. the argument checks ------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_every_entry_is_written():
    lib = T.load()
    pos = torch.from_numpy(np.ascontiguousarray(np.concatenate([hand_records(), hand_records()]))).to(DEV)
    before = pos.clone()
    out = [torch.full(shape, 77, dtype=torch.int32, device=DEV) for shape in ((2, 81), (2, 81), (2, 81), (2, 163), (2,))]
    ptr = [x.data_ptr() for x in out]

    def call(p=pos.data_ptr(), records=2, playouts=3, komi=KOMI, b=ptr[0], w=ptr[1], a=ptr[2], h=ptr[3], bw=ptr[4]):
        return lib.bkt_owner_counts(p, records, playouts, komi, b, w, a, h, bw, None)

    for kw in (dict(p=None), dict(b=None), dict(w=None), dict(a=None), dict(h=None), dict(bw=None),       # a NULL pointer
               dict(records=0), dict(records=-2), dict(playouts=0), dict(playouts=-1),                    # nothing to do
               dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30),    # too many rows
               dict(komi=float("inf")), dict(komi=float("-inf")), dict(komi=float("nan"))):               # no komi
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all((x == 77).all().item() for x in out)
    assert call() == 0
    torch.cuda.synchronize()
    same_counts(tuple(x.cpu().numpy() for x in out), tuple(np.concatenate([x, x]) for x in HAND))    # zeros included
    assert torch.equal(pos, before)
    for bad in ((pos, 2, 4), (pos, 0, 3), (pos, 3, 0), (pos.to(torch.int8), 2, 3), (pos.cpu(), 2, 3), (pos[:, :191], 2, 3),
                (pos, 2, 3, float("nan")), (pos, 2, 3, float("inf"))):
        with pytest.raises(ValueError):
            T.owner_counts(*bad)


# ---- 3. whole playouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_tables", [False, True])
def test_playout_ownership_equals_the_host_rules_and_the_value(five, with_tables):
    kw = dict(zip(("patterns", "tactics"), seeded_tables())) if with_tables else {}
    host = RO.playout_ownership(five, 7, SEED, rules="host", **kw)
    dev = RO.playout_ownership(five, 7, SEED, rules="device", **kw)
    same_counts(tuple(getattr(dev, f) for f in COUNTS), tuple(getattr(host, f) for f in COUNTS))
    assert dev.n == host.n == 7 and dev.wins.dtype == host.wins.dtype == np.int32 and np.array_equal(dev.wins, host.wins)
    value = RO.playout_value(five, 7, SEED, rules="device", **kw)
    assert dev.value.dtype == np.float32 and np.array_equal(dev.value.view(np.int32), value.view(np.int32))
    assert np.array_equal(host.value.view(np.int32), value.view(np.int32))
    assert np.array_equal(dev.criticality(), host.criticality()) and np.array_equal(dev.mean_owner, host.mean_owner)
    assert dev.black_wins[0] == 7 and dev.hist[0, 90] == 7 and dev.hist.sum(1).tolist() == [7] * 5
    on_device = RO.playout_ownership(torch.from_numpy(five).to(DEV), 7, SEED, **kw)    # records that are there already
    same_counts(tuple(getattr(on_device, f) for f in COUNTS), tuple(getattr(host, f) for f in COUNTS))
    if with_tables:                                                       # (the tables do change the games)
        plain = RO.playout_ownership(five, 7, SEED)
        assert not np.array_equal(plain.black, dev.black)
        pat = RO.playout_ownership(five, 7, SEED, patterns=kw["patterns"])
        assert np.array_equal(pat.value.view(np.int32), RO.playout_value(five, 7, SEED, patterns=kw["patterns"]).view(np.int32))


# ---- 4. the evaluator, the tree and GTP ----------------------------------------------------------------------------------------------
def test_the_criticality_evaluator_equals_the_host_rules(five):
    recs = np.ascontiguousarray(np.concatenate([five, five[1:2]]))
    for rave in (False, True):
        dev, host = (RO.PlayoutEvaluator(None, 7, seed=SEED, prior=1.0, criticality=1.0, rave=rave, rules=rules)
                     for rules in ("device", "host"))
        out_d, out_h = dev(recs, 2), host(recs, 2)
        assert len(out_d) == len(out_h) == 2 + rave
        assert out_d[0].shape == (2, 81) and np.array_equal(out_d[0].view(np.int32), out_h[0].view(np.int32))
        assert np.array_equal(out_d[1].view(np.int32), out_h[1].view(np.int32))
        plain = RO.PlayoutEvaluator(None, 7, seed=SEED, prior=1.0, rave=rave)(recs, 2)
        assert np.array_equal(plain[1], out_d[1]) and not np.array_equal(plain[0][1], out_d[0][1])
        if rave:
            assert out_d[2][0] == out_h[2][0] == 7
            for d, h, p in zip(out_d[2][1:], out_h[2][1:], plain[2][1:]):
                assert np.array_equal(d, h) and np.array_equal(d, p)
    a = RO.playout_amaf(recs[:2], 7, SEED)
    o = RO.playout_ownership(recs[:2], 7, SEED)
    from bokego_amd.selfplay import normalise_like_categorical
    want = normalise_like_categorical(RO.amaf_prior(recs[:2], a, criticality=o.criticality(), gamma=1.0))
    assert np.array_equal(out_d[0].view(np.int32), want.view(np.int32))


def test_native_mcts_with_criticality_device_against_host_rules():
    """A late middle game (58 stones), so that the host rules' playouts are short: 60 rollouts, net-free, RAVE on."""
    r = max(_golden(), key=lambda r: sum(c != "." for c in r["board"]))
    seen = []
    for rules in ("device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=8, playout_prior=1, playout_criticality=1, playout_rave=4, expand_thresh=3,
                       playout_seed=SEED, playout_rules=rules)
        assert t.evaluator.rules == rules and t.evaluator.rave and t.evaluator.criticality == 1.0
        t.rollout(60)
        stats = {mv: n for mv, (n, _) in t.child_stats().items()}
        seen.append((stats, t.choose().last_move))
        t.close()
    assert seen[0] == seen[1]
    assert sum(seen[0][0].values()) == 60 and seen[0][1] in seen[0][0]


def test_gtp_without_a_net_lists_the_dead_stone():
    g = gtp.NativeGTP(Position(board=DEAD), None, None, no_sim=True, time_lim=None, n_rollouts=8, playout_value=8,
                      playout_prior=1.0, rollout_score=16, rollout_seed=SEED)
    assert g.policy_net is None and g.evaluator.rules == "device"
    g.running = True
    assert g.send("final_status_list dead") == f"= {go.unsquash(37)}\n\n"
    assert g.send("final_status_list seki") == "= \n\n"
    assert g.send("final_score") == "= B+3.5\n\n"
    alive = g.send("final_status_list alive").split()[1:]
    assert len(alive) == sum(c != "." for c in DEAD) - 1 and go.unsquash(37) not in alive
    host = RO.ownership_score([go.Game(DEAD)], 16, SEED, rules="host")[0]
    assert host.stones("dead") == [37] and host.score == 3.5
    g.close()

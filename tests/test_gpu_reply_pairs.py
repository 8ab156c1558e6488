"""Replies keyed by the last two moves on the GPU: bkt_reply2_playouts and the event-parallel bkt_reply2_update
against the host mirror, byte for byte, and the evaluator and the tree search end to end."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import seeded_tables
from test_pattern_prior_cpu import golden_records
from test_replies_cpu import random_histories, start
from test_reply_pairs_cpu import (HAND2_AFTER, HAND2_BEFORE, HAND2_MOVES, HAND2_RECS, HAND2_WON, NO, NONE, S, learned_nine,
                                  nine_records, random_table2)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
CAPS = (1, 2, 8, RO.MAX_PLIES)
COMBOS = {"uniform": (False, False), "patterns": (True, False), "tactics": (False, True), "both": (True, True)}
SCRATCH = 119556


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


@pytest.fixture(scope="module")
def nine():
    return nine_records()


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def pair_tables():
    """All 255; plane 81 of the learned table alone; the learned table; and the learned table with 81s and 200s planted."""
    full = learned_nine().array
    singles = np.full_like(full, NO)
    singles[:, S] = full[:, S]
    planted = full.copy()
    rng = np.random.default_rng(8)
    planted[rng.random(planted.shape) < 0.3] = 81
    planted[rng.random(planted.shape) < 0.3] = 200
    assert (planted <= 80).sum() > 100
    return {"empty": np.full_like(full, NO), "singles": singles, "learned": full, "planted": planted}


@pytest.fixture(scope="module")
def mirror(nine, tables, pair_tables):
    """The host playouts of the nine records, once per table combination, pair table and cap: a row's game depends on its
    record, its counters and the tables alone, so every batch below is compared with the first rows of these."""
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(9, RO.record_turns(nine)), 9)
    out = {}
    for combo, (p, t) in COMBOS.items():
        for which, table in pair_tables.items():
            for cap in CAPS:
                out[combo, which, cap] = RO._random_host(nine, key, ctr, cap, L.KOMI, True, tables[0] if p else None,
                                                         tables[1] if t else None, RO.ReplyTable2(table))
    return out


def launch(recs, combo, tables, replies2, cap, over=None, rows=None, single=None):
    """T.reply2_playouts (or, with single, T.reply_playouts) on the first rows of recs with the counters of those rows
    -> (records, over, plies, moves, status)."""
    B = len(recs) if rows is None else rows
    pos = dev(recs[:B])
    ctr = dev(RO.default_counters(len(recs), RO.record_turns(recs))[:B])
    p, t = COMBOS[combo]
    args = (tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None)
    if single is not None:
        out = T.reply_playouts(pos, SEED, ctr, *args, dev(single), cap, over=over)
    else:
        out = T.reply2_playouts(pos, SEED, ctr, *args, dev(replies2), cap, over=over)
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


# ---- 1. bkt_reply2_playouts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", list(COMBOS))
def test_playouts_equal_the_mirror_byte_for_byte(nine, tables, pair_tables, mirror, combo):
    for which, table in pair_tables.items():
        for cap in CAPS:
            want = mirror[combo, which, cap]
            for B in (1, 2, 3, 4, 7):                                 # one seat; tails with two idle seats and one; full + 1
                recs, over, plies, moves, status = launch(nine, combo, tables, table, cap, rows=B)
                what = (combo, which, cap, B)
                assert np.array_equal(recs, want.records[:B]), what
                assert np.array_equal(over != 0, want.over[:B]) and np.array_equal(plies, want.plies[:B]), what
                assert moves.shape == (B, cap) and not status.any(), what
                width = want.moves.shape[1]                          # the mirror's history is cut to its longest game
                assert np.array_equal(moves[:, :width], want.moves[:B]) and (moves[:, width:] == NONE).all(), what
            if which == "singles":                                    # no pair anywhere: bkt_reply_playouts with plane 81
                single = np.ascontiguousarray(table[:, S])
                for got, sib in zip(launch(nine, combo, tables, table, cap), launch(nine, combo, tables, None, cap, single=single)):
                    assert np.array_equal(got, sib), (combo, cap)
    full, singles = mirror[combo, "learned", RO.MAX_PLIES], mirror[combo, "singles", RO.MAX_PLIES]
    assert full.reply_pair_plies > 0 and singles.reply_pair_plies == 0 and singles.reply_plies > 0
    assert mirror[combo, "empty", RO.MAX_PLIES].reply_plies == 0 and mirror[combo, "planted", 8].reply_plies > 0
    assert not np.array_equal(full.moves, singles.moves[:, :full.moves.shape[1]]) or full.moves.shape != singles.moves.shape


def test_a_row_over_on_entry(nine, tables, pair_tables):
    over = torch.zeros((9,), dtype=torch.uint8, device=DEV)
    over[1] = over[4] = 1
    recs, o, plies, moves, status = launch(nine, "both", tables, pair_tables["learned"], RO.MAX_PLIES, over=over)
    assert np.array_equal(recs[[1, 4]], nine[[1, 4]]) and (moves[[1, 4]] == NONE).all() and not plies[[1, 4]].any()
    assert o[1] == 1 and o[4] == 1 and not status.any() and plies[2] > 2
    free = launch(nine, "both", tables, pair_tables["learned"], RO.MAX_PLIES)
    keep = [0, 2, 3, 5, 6, 7, 8]                                      # the other rows play the games they play anyway
    assert np.array_equal(recs[keep], free[0][keep]) and np.array_equal(moves[keep], free[3][keep])


def test_refused_playout_calls_write_nothing(nine):
    lib = T.load()
    pos, ctr = dev(nine), dev(RO.default_counters(9, RO.record_turns(nine)))
    over = torch.full((9,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((9,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((9, 8), 77, dtype=torch.int16, device=DEV)
    buf = torch.full((13284 + 8,), NO, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0

    def call(p=pos.data_ptr(), batch=9, c=ctr.data_ptr(), r=buf.data_ptr(), cap=8, o=over.data_ptr(), n=plies.data_ptr(),
             s=status.data_ptr()):
        return lib.bkt_reply2_playouts(p, batch, SEED, c, None, None, r, cap, o, n, moves.data_ptr(), s, None)

    for kw in (dict(r=None), dict(r=buf.data_ptr() + 1), dict(r=buf.data_ptr() + 2), dict(r=buf.data_ptr() + 3), dict(p=None),
               dict(c=None), dict(o=None), dict(n=None), dict(s=None), dict(batch=0), dict(batch=T.MAX_BATCH + 1), dict(cap=0),
               dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), nine) and (over == 7).all().item() and (moves == 77).all().item()
    assert (plies == 77).all().item() and (status == 77).all().item()
    assert call(r=buf.data_ptr() + 4) == 0                             # 4-byte aligned is enough
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    with pytest.raises(ValueError):
        T.reply2_playouts(pos, SEED, ctr, None, None, buf[:162].view(2, 81), 8)


# ---- 2. bkt_reply2_update -------------------------------------------------------------------------------------------------------
def update(table, recs, moves, won, records, playouts, times=1):
    """T.reply2_update on a table between guard bytes, with a sentinel-filled scratch and guard bytes behind it
    -> uint8 [2,82,81]."""
    assert T.load().bkt_reply2_scratch_bytes() == SCRATCH
    buf = torch.full((256 + 13284 + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    mine = buf[256:256 + 13284].view(2, 82, 81)
    mine.copy_(dev(table))
    scratch = torch.full((SCRATCH + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    for _ in range(times):
        T.reply2_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, mine, scratch)
    assert (buf[:256] == 0x5A).all().item() and (buf[256 + 13284:] == 0x5A).all().item()
    assert (scratch[SCRATCH:] == 0xA5).all().item()
    return mine.cpu().numpy()


def test_update_equals_the_hand_written_fold():
    assert np.array_equal(update(HAND2_BEFORE, HAND2_RECS, HAND2_MOVES, HAND2_WON, 4, 3), HAND2_AFTER)
    rows = np.repeat(HAND2_RECS, 3, 0)                                # and as twelve records of one playout each
    assert np.array_equal(update(HAND2_BEFORE, rows, HAND2_MOVES, HAND2_WON, 12, 1), HAND2_AFTER)


@pytest.fixture(scope="module")
def real(nine):
    """64 uniform playouts of 82 records at both caps, on the device: histories and winners (the tests take the first
    playouts of a record's 64)."""
    gold = golden_records()
    recs = np.ascontiguousarray(np.concatenate([nine, gold[::max(len(gold) // 73, 1)][:73]]))
    assert len(recs) == 82
    out = {}
    for cap in (8, 400):
        pos = dev(recs).repeat_interleave(64, 0)
        moves = T.random_playouts(pos, SEED, L.value_counters_device(dev(recs), 64), cap)[2]
        won = (T.area_score(pos, L.KOMI) > 0).view(82, 64) == L.black_to_move(dev(recs))[:, None]
        out[cap] = (moves.cpu().numpy(), won.reshape(-1).cpu().numpy().astype(np.uint8))
    return recs, out


@pytest.mark.parametrize("cap", [8, 400])
@pytest.mark.parametrize("records,playouts", [(1, 1), (1, 3), (2, 64), (5, 7), (82, 8)])
def test_update_equals_the_mirror_on_real_histories(real, records, playouts, cap):
    recs, runs = real
    moves, won = runs[cap]
    first = 1 if records < 3 else 0                                   # (record 0 needs no luck: every playout is one move)
    pick = np.arange(first, first + records) if records < 82 else np.arange(82)
    rows = (pick[:, None] * 64 + np.arange(playouts)[None, :]).reshape(-1)
    rng = np.random.default_rng(records * 100 + playouts)
    before = rng.integers(0, 81, (2, 82, 81)).astype(np.uint8)        # a random table, so that clears find something
    before[rng.random(before.shape) < 0.3] = NO
    before[1, 40, 40], before[0, S, 3] = 200, 81                      # invalid values
    want = before.copy()
    events = RO.reply2_update_host(want, recs[pick], moves[rows], won[rows], records, playouts)
    got = update(before, recs[pick], moves[rows], won[rows], records, playouts)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:8], events)
    assert events[0] > 0 and (records * playouts < 8 or cap == 8 or events[1] > 0)
    single = np.ascontiguousarray(before[:, S])                       # plane 81 is what bkt_reply_update leaves
    T.reply_update(dev(recs[pick]), dev(moves[rows]), dev(won[rows], torch.uint8), records, playouts, s := dev(single))
    assert np.array_equal(got[:, S], s.cpu().numpy())


@pytest.mark.parametrize("max_plies", [1, 2, 63, 64, 65, 400, 1024])
def test_update_equals_the_mirror_on_colliding_histories(max_plies):
    recs, moves, won = random_histories(3, 5, max_plies, 40 + max_plies)
    want = random_table2(9)
    RO.reply2_update_host(want, recs, moves, won, 3, 5)
    got = update(random_table2(9), recs, moves, won, 3, 5)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    # 15 rows are no multiple of the four rows of a workgroup; neither are 5 and 13
    for records, playouts in ((1, 5), (13, 1)):
        recs, moves, won = random_histories(records, playouts, max_plies, 70 + max_plies)
        want = random_table2(10)
        RO.reply2_update_host(want, recs, moves, won, records, playouts)
        assert np.array_equal(update(random_table2(10), recs, moves, won, records, playouts), want)


def test_nothing_after_the_end_of_a_row_counts():
    recs = np.stack([start(40, 0), start(12, 1)])
    rng = np.random.default_rng(3)
    moves = rng.integers(0, 9, (6, 200)).astype(np.int16)
    moves[:, 70] = NONE                                               # the end, in the second chunk of 64
    moves[:, 71:128] = NONE
    assert (moves[:, 128:] >= 0).all()                                # valid-looking moves from ply 128 on, the third chunk
    moves[1, 70:] = rng.integers(0, 9, 130)                           # one row that does go on
    won = np.array([1, 0, 1, 0, 1, 0], np.uint8)
    want = random_table2(5, points=9)
    RO.reply2_update_host(want, recs, moves, won, 2, 3)
    cut = moves.copy()
    cut[[0, 2, 3, 4, 5], 71:] = NONE
    same = random_table2(5, points=9)
    RO.reply2_update_host(same, recs, cut, won, 2, 3)
    assert np.array_equal(want, same)
    assert np.array_equal(update(random_table2(5, points=9), recs, moves, won, 2, 3), want)


def test_updates_back_to_back_twice_and_the_argument_checks():
    a, b = random_histories(3, 5, 9, 1), random_histories(2, 7, 30, 2)
    want = random_table2(4)
    RO.reply2_update_host(want, *a, 3, 5)
    RO.reply2_update_host(want, *b, 2, 7)
    replies = dev(random_table2(4))
    scratch = torch.empty((SCRATCH,), dtype=torch.uint8, device=DEV)   # one scratch for both: the stream orders the launches
    args = [(dev(r), dev(m), dev(w), n, k) for (r, m, w), n, k in ((a, 3, 5), (b, 2, 7))]
    for r, m, w, n, k in args:                                        # queued without a wait in between
        T.reply2_update(r, m, w, n, k, replies, scratch)
    assert np.array_equal(replies.cpu().numpy(), want)
    # the same update twice from the same start: the same bytes
    first, second = (update(random_table2(4), *b, 2, 7) for _ in range(2))
    assert np.array_equal(first, second)
    lib = T.load()
    r, m, w, _, _ = args[0]
    buf = torch.full((13284 + 8,), 0x11, dtype=torch.uint8, device=DEV)
    scratch = torch.full((SCRATCH + 8,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=9, wn=w.data_ptr(), records=3, playouts=5, t=buf.data_ptr(),
             s=scratch.data_ptr()):
        return lib.bkt_reply2_update(p, mv, cap, wn, records, playouts, t, s, None)

    for kw in (dict(p=None), dict(mv=None), dict(wn=None), dict(t=None), dict(s=None), dict(t=buf.data_ptr() + 1),
               dict(t=buf.data_ptr() + 2), dict(s=scratch.data_ptr() + 4), dict(records=0), dict(records=-2), dict(playouts=0),
               dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30),
               dict(cap=0), dict(cap=-8), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (buf == 0x11).all().item() and (scratch == 0xA5).all().item()
    with pytest.raises(ValueError):
        T.reply2_update(r, m, w, 3, 5, replies, scratch[:100])
    with pytest.raises(ValueError):
        T.reply2_update(r, m, w, 3, 5, replies[:, S].contiguous())


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
def test_the_evaluator_equals_the_host_rules_request_for_request(nine):
    recs = np.ascontiguousarray(nine[[1, 2, 3, 4, 5]])
    same = lambda x: x                                                # noqa: E731
    more = dict(rave=True, criticality=0.5)
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rules=rules, replies=2, **more) for rules in ("device", "host")]
    values = []
    for k in range(3):
        d, h = (ev.finish(ev.submit(recs, 2), normalise=same) for ev in evs)
        assert len(d) == len(h) == 3
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        values.append(d[1])
    assert evs[0].replies.pairs_occupancy() > 0 and not np.array_equal(values[0], values[2])
    # two requests in flight see the table in submit order
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, replies=2, **more)
    h1, h2 = ev.submit(recs, 2), ev.submit(recs, 2)
    assert np.array_equal(ev.finish(h2, normalise=same)[1], values[1]) and np.array_equal(ev.finish(h1, normalise=same)[1], values[0])
    # the functions that take a table
    t_dev, t_host = RO.ReplyTable2.empty(), RO.ReplyTable2.empty()
    for _ in range(2):
        a, b = (RO.playout_amaf(recs, 6, SEED, rules=rules, replies=t, sides=2) for rules, t in (("device", t_dev), ("host", t_host)))
        assert np.array_equal(a.value.view(np.int32), b.value.view(np.int32)) and np.array_equal(a.played, b.played)
        assert np.array_equal(t_dev.array, t_host.array)
    f_dev, f_host = (RO.random_playouts(recs, SEED, rules=rules, replies=t) for rules, t in (("device", t_dev), ("host", t_host)))
    assert np.array_equal(f_dev.moves, f_host.moves) and np.array_equal(t_dev.array, t_host.array)
    assert f_dev.reply_plies is None and f_dev.reply_pair_plies is None and f_host.reply_pair_plies > 0


def test_native_mcts_with_reply_pairs_equals_the_host_rules():
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][60]   # a mid-game position: shorter playouts
    seen = []
    for rules in ("device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=4, playout_prior=1.0, playout_rave=4, playout_reply_pairs=True, playout_seed=SEED,
                       playout_rules=rules, expand_thresh=2)
        assert t.evaluator.rules == rules and type(t.evaluator.replies) is RO.ReplyTable2
        t.rollout(60)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move, t.evaluator.replies.array.copy()))
        t.close()
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1] and sum(seen[0][0].values()) == 60
    assert np.array_equal(seen[0][2], seen[1][2]) and (seen[0][2][:, :S] != NO).sum() > 10

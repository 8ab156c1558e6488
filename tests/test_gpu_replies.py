"""The last-good-reply playouts and their table's update on the GPU: bkt_reply_playouts and bkt_reply_update
against the host mirror, byte for byte, and the evaluator and the tree search end to end."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import replies as RP
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import seeded_tables, three_records
from test_pattern_prior_cpu import eyes_only_record, golden_records, ko_record
from test_replies_cpu import (HAND_AFTER, HAND_BEFORE, HAND_MOVES, HAND_RECS, HAND_WON, NO, learned, random_histories,
                              random_table)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
CAPS = (1, 8, RO.MAX_PLIES)
COMBOS = {"uniform": (False, False), "patterns": (True, False), "tactics": (False, True), "both": (True, True)}


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


@pytest.fixture(scope="module")
def nine():
    """The five records of test_gpu_amaf.py (the board that needs no luck, the empty board, a record after a pass, two
    mid-game goldens, one per colour), the ko record and the eyes-only board (white to move in both), and two more goldens."""
    gold = golden_records()
    black = L.black_to_move(gold)
    mid = np.stack([gold[60], gold[61 + int(np.argmax(black[61:] != black[60]))]])
    recs = np.ascontiguousarray(np.concatenate([three_records(), mid, ko_record(), eyes_only_record(), gold[30:32]]))
    assert len(recs) == 9 and (~L.black_to_move(recs)).sum() >= 3
    return recs


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def reply_tables(nine):
    """All 255, and a table learned from four uniform playouts of each of the nine records."""
    table, (n_set, n_cleared, _), _ = learned(nine, 4, SEED)
    assert n_set > 0 and n_cleared > 0 and table.occupancy() > 20
    return {"empty": RO.ReplyTable.empty(), "learned": table}


@pytest.fixture(scope="module")
def mirror(nine, tables, reply_tables):
    """The host playouts of the nine records, once per table combination, reply table and cap: a row's game depends on its
    record, its counters and the tables alone, so every batch below is compared with the first rows of these."""
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(9, RO.record_turns(nine)), 9)
    out = {}
    for combo, (p, t) in COMBOS.items():
        for which, table in reply_tables.items():
            for cap in CAPS:
                out[combo, which, cap] = RO._random_host(nine, key, ctr, cap, L.KOMI, True, tables[0] if p else None,
                                                         tables[1] if t else None, table.copy())
    return out


def launch(recs, combo, tables, replies, cap, over=None, rows=None):
    """T.reply_playouts on the first rows of recs with the counters of those rows -> (records, over, plies, moves, status)."""
    B = len(recs) if rows is None else rows
    pos = dev(recs[:B])
    ctr = dev(RO.default_counters(len(recs), RO.record_turns(recs))[:B])
    p, t = COMBOS[combo]
    args = (tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None)
    if replies is None:
        play = (T.tactical_playouts if t else T.pattern_playouts if p else T.random_playouts)
        out = play(pos, SEED, ctr, *(args if t else args[:1] if p else ()), cap, over=over)
    else:
        out = T.reply_playouts(pos, SEED, ctr, *args, dev(replies), cap, over=over)
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


# ---- 1. bkt_reply_playouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", list(COMBOS))
def test_playouts_equal_the_mirror_byte_for_byte(nine, tables, reply_tables, mirror, combo):
    for which, table in reply_tables.items():
        for cap in CAPS:
            want = mirror[combo, which, cap]
            for B in (1, 2, 3, 4, 7, 9):                              # one seat; tails with two idle seats and one; full + 1
                recs, over, plies, moves, status = launch(nine, combo, tables, table.array, cap, rows=B)
                what = (combo, which, cap, B)
                assert np.array_equal(recs, want.records[:B]), what
                assert np.array_equal(over != 0, want.over[:B]) and np.array_equal(plies, want.plies[:B]), what
                assert moves.shape == (B, cap) and not status.any(), what
                width = want.moves.shape[1]                          # the mirror's history is cut to its longest game
                assert np.array_equal(moves[:, :width], want.moves[:B]) and (moves[:, width:] == RO.MOVE_NONE).all(), what
            if which == "empty":                                      # the wrapper alone: the sibling kernel's bytes
                for got, sib in zip(launch(nine, combo, tables, table.array, cap), launch(nine, combo, tables, None, cap)):
                    assert np.array_equal(got, sib), (combo, cap)
    full, empty = mirror[combo, "learned", RO.MAX_PLIES], mirror[combo, "empty", RO.MAX_PLIES]
    assert full.reply_plies > 0 and empty.reply_plies == 0
    assert full.reply_plies == RP.reply_plies_of(reply_tables["learned"], nine, full.moves, 1)
    assert (full.moves[:, :8] != empty.moves[:, :8]).any()           # the learned table did change games


def test_a_row_over_on_entry_and_a_table_of_invalid_values(nine, tables):
    over = torch.zeros((9,), dtype=torch.uint8, device=DEV)
    over[1] = over[4] = 1
    table = np.full((2, 81), NO, np.uint8)
    recs, o, plies, moves, status = launch(nine, "both", tables, table, RO.MAX_PLIES, over=over)
    assert np.array_equal(recs[[1, 4]], nine[[1, 4]]) and (moves[[1, 4]] == RO.MOVE_NONE).all() and not plies[[1, 4]].any()
    assert o[1] == 1 and o[4] == 1 and not status.any() and plies[2] > 2
    plain = launch(nine, "both", tables, table, 8)
    table[:] = np.arange(162).reshape(2, 81) % 93 + 81                # every value above 80: 81..173, never an index
    table[table == NO] = 254
    for got, want in zip(launch(nine, "both", tables, table, 8), plain):
        assert np.array_equal(got, want)


def test_a_null_table_is_refused_and_nothing_is_written(nine):
    lib = T.load()
    pos, ctr = dev(nine), dev(RO.default_counters(9, RO.record_turns(nine)))
    over = torch.full((9,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((9,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((9, 8), 77, dtype=torch.int16, device=DEV)
    replies = dev(np.full((2, 81), NO, np.uint8))

    def call(p=pos.data_ptr(), batch=9, c=ctr.data_ptr(), r=replies.data_ptr(), cap=8, o=over.data_ptr(), n=plies.data_ptr(),
             s=status.data_ptr()):
        return lib.bkt_reply_playouts(p, batch, SEED, c, None, None, r, cap, o, n, moves.data_ptr(), s, None)

    for kw in (dict(r=None), dict(p=None), dict(c=None), dict(o=None), dict(n=None), dict(s=None), dict(batch=0),
               dict(batch=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), nine) and (over == 7).all().item() and (moves == 77).all().item()
    assert (plies == 77).all().item() and (status == 77).all().item()


# ---- 2. bkt_reply_update --------------------------------------------------------------------------------------------------------
def update(table, recs, moves, won, records, playouts, check_guards=True):
    """T.reply_update on a table between guard rows, with a sentinel-filled scratch and guard bytes behind it -> uint8 [2,81]."""
    buf = torch.full((4, 81), 0x5A, dtype=torch.uint8, device=DEV)
    buf[1:3] = dev(table)
    need = T.load().bkt_reply_scratch_bytes(records)
    assert need == records * 2592
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    T.reply_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, buf[1:3], scratch)
    if check_guards:
        assert (buf[0] == 0x5A).all().item() and (buf[3] == 0x5A).all().item() and (scratch[need:] == 0xA5).all().item()
    return buf[1:3].cpu().numpy()


def test_update_equals_the_hand_written_fold():
    assert np.array_equal(update(HAND_BEFORE, HAND_RECS, HAND_MOVES, HAND_WON, 4, 3), HAND_AFTER)
    rows = np.repeat(HAND_RECS, 3, 0)                                 # and as twelve records of one playout each
    assert np.array_equal(update(HAND_BEFORE, rows, HAND_MOVES, HAND_WON, 12, 1), HAND_AFTER)


@pytest.fixture(scope="module")
def real(nine):
    """64 uniform playouts of 82 records at both caps, on the device: histories and winners."""
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
@pytest.mark.parametrize("records,playouts", [(1, 1), (1, 3), (2, 64), (5, 7), (82, 64)])
def test_update_equals_the_mirror_on_real_histories(real, records, playouts, cap):
    recs, runs = real
    moves, won = runs[cap]
    first = 1 if records < 3 else 0                                   # (record 0 needs no luck: every playout is one move)
    pick = np.arange(first, first + records) if records < 82 else np.arange(82)
    rows = (pick[:, None] * 64 + np.arange(playouts)[None, :]).reshape(-1)
    rng = np.random.default_rng(records * 100 + playouts)
    before = rng.integers(0, 81, (2, 81)).astype(np.uint8)
    before[rng.random((2, 81)) < 0.3] = NO
    before[1, 40] = 200                                               # one invalid value
    want = before.copy()
    events = RO.reply_update_host(want, recs[pick], moves[rows], won[rows], records, playouts)
    got = update(before, recs[pick], moves[rows], won[rows], records, playouts)
    assert np.array_equal(got, want), (np.nonzero(got != want), events)
    assert events[0] > 0 and (records * playouts < 8 or cap == 8 or events[1] > 0)


@pytest.mark.parametrize("records,playouts,max_plies", [(3, 9, 37), (7, 4, 401), (2, 6, 3), (1, 5, 1024)])
def test_update_equals_the_mirror_on_any_history(records, playouts, max_plies):
    recs, moves, won = random_histories(records, playouts, max_plies, 40 + records)
    want = random_table(9)
    RO.reply_update_host(want, recs, moves, won, records, playouts)
    assert np.array_equal(update(random_table(9), recs, moves, won, records, playouts), want)


def test_two_updates_back_to_back_and_the_argument_checks():
    a, b = random_histories(3, 5, 9, 1), random_histories(2, 7, 30, 2)
    want = random_table(4)
    RO.reply_update_host(want, *a, 3, 5)
    RO.reply_update_host(want, *b, 2, 7)
    replies = dev(random_table(4))
    scratch = torch.empty((3 * 2592,), dtype=torch.uint8, device=DEV)  # one scratch for both: the stream orders the four launches
    args = [(dev(r), dev(m), dev(w), n, k) for (r, m, w), n, k in ((a, 3, 5), (b, 2, 7))]
    for r, m, w, n, k in args:                                        # queued without a wait in between
        T.reply_update(r, m, w, n, k, replies, scratch)
    assert np.array_equal(replies.cpu().numpy(), want)
    lib = T.load()
    r, m, w, _, _ = args[0]
    replies, scratch = dev(HAND_BEFORE), torch.full((3 * 2592,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=9, wn=w.data_ptr(), records=3, playouts=5, t=replies.data_ptr(),
             s=scratch.data_ptr()):
        return lib.bkt_reply_update(p, mv, cap, wn, records, playouts, t, s, None)

    for kw in (dict(p=None), dict(mv=None), dict(wn=None), dict(t=None), dict(s=None), dict(records=0), dict(records=-2),
               dict(playouts=0), dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1),
               dict(records=1 << 30, playouts=1 << 30), dict(cap=0), dict(cap=-8), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(replies.cpu().numpy(), HAND_BEFORE) and (scratch == 0xA5).all().item()
    with pytest.raises(ValueError):
        T.reply_update(r, m, w, 3, 5, replies, scratch[:100])


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", [dict(), dict(rave=True, criticality=0.5)], ids=["plain", "rave-criticality"])
def test_the_evaluator_equals_the_host_rules_request_for_request(nine, more):
    recs = np.ascontiguousarray(nine[[1, 2, 3, 4, 5]])
    same = lambda x: x                                                # noqa: E731
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rules=rules, replies=True, **more) for rules in ("device", "host")]
    values = []
    for k in range(3):
        d, h = (ev.finish(ev.submit(recs, 2), normalise=same) for ev in evs)
        assert len(d) == len(h) == 2 + bool(more)
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        if more:
            assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        values.append(d[1])
    assert evs[0].replies.occupancy() > 0 and not np.array_equal(values[0], values[2])
    # two requests in flight see the table in submit order
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, replies=True, **more)
    h1, h2 = ev.submit(recs, 2), ev.submit(recs, 2)
    assert np.array_equal(ev.finish(h2, normalise=same)[1], values[1]) and np.array_equal(ev.finish(h1, normalise=same)[1], values[0])
    # the functions that take a table
    t_dev, t_host = RO.ReplyTable.empty(), RO.ReplyTable.empty()
    for _ in range(2):
        a, b = (RO.playout_amaf(recs, 6, SEED, rules=rules, replies=t, sides=2) for rules, t in (("device", t_dev), ("host", t_host)))
        assert np.array_equal(a.value.view(np.int32), b.value.view(np.int32)) and np.array_equal(a.played, b.played)
        assert np.array_equal(t_dev.array, t_host.array)
    f_dev, f_host = (RO.random_playouts(recs, SEED, rules=rules, replies=t) for rules, t in (("device", t_dev), ("host", t_host)))
    assert np.array_equal(f_dev.moves, f_host.moves) and np.array_equal(t_dev.array, t_host.array) and f_dev.reply_plies is None
    with pytest.raises(ValueError, match="scored"):
        RO.playout_ownership(recs, 4, SEED, replies=t_dev)


def test_native_mcts_with_replies_equals_the_host_rules(nine):
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][60]   # a mid-game position: shorter playouts
    seen = []
    for rules in ("device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=4, playout_prior=1.0, playout_rave=4, playout_replies=True, playout_seed=SEED,
                       playout_rules=rules, expand_thresh=2)
        assert t.evaluator.rules == rules and isinstance(t.evaluator.replies, RO.ReplyTable)
        t.rollout(60)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move, t.evaluator.replies.array.copy()))
        t.close()
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1] and sum(seen[0][0].values()) == 60
    assert np.array_equal(seen[0][2], seen[1][2]) and (seen[0][2] != NO).sum() > 10

"""MAST playouts on the GPU: bkt_move_value_playouts against the host mirror and, with neutral values, against
every entry point it wraps, byte for byte; bkt_move_value_update against the mirror integer for integer; and the
evaluator and the tree search end to end."""
import json
import os

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import movevalues as MV
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import seeded_tables
from test_mast_cpu import HAND_MOVES, HAND_RECS, HAND_WON, learned_values, ramp_lut
from test_pattern_prior_cpu import golden_records
from test_replies_cpu import random_histories
from test_reply_pairs_cpu import NONE, S, learned_nine, nine_records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
CAPS = (1, 8, RO.MAX_PLIES)
COMBOS = {"uniform": (False, False), "patterns": (True, False), "tactics": (False, True), "both": (True, True)}
FORMS = ("none", "single", "pairs")


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def bits(x):
    return dev(np.array(x, np.uint16).view(np.int16))              # (a copy: a table's lut is read-only)


@pytest.fixture(scope="module")
def nine():
    return nine_records()


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def replies():
    """The learned pair table and its plane 81 as a single table."""
    pairs = learned_nine().array
    return {"none": None, "single": np.ascontiguousarray(pairs[:, S]), "pairs": pairs}


@pytest.fixture(scope="module")
def random_values():
    v = np.random.default_rng(30).integers(1, 65536, (2, 81)).astype(np.uint16)
    v[0, ::7], v[1, 3::5], v[:, 40] = 1, 65535, (65535, 1)
    return v


def table_with(values):
    return MV.MoveValueTable(np.zeros((2, 81, 2), np.int64), values, MV.lut_of(1.0), 1, 0)


def host_games(recs, tables, combo, values, form, replies, cap):
    p, t = COMBOS[combo]
    table = {"none": None, "single": RO.ReplyTable, "pairs": RO.ReplyTable2}[form]
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(len(recs), RO.record_turns(recs)), len(recs))
    return RO._random_host(recs, key, ctr, cap, L.KOMI, True, tables[0] if p else None, tables[1] if t else None,
                           None if table is None else table(replies[form]), None, table_with(values))


def launch(recs, tables, combo, values, form, replies, cap, over=None, rows=None):
    """T.move_value_playouts on the rows `rows` (an index array; default all) of recs with the counters of those rows
    -> (records, over, plies, moves, status)."""
    rows = np.arange(len(recs)) if rows is None else np.asarray(rows)
    pos = dev(recs[rows])
    ctr = dev(RO.default_counters(len(recs), RO.record_turns(recs))[rows])
    p, t = COMBOS[combo]
    put = {} if form == "none" else {"replies" if form == "single" else "replies2": dev(replies[form])}
    out = T.move_value_playouts(pos, SEED, ctr, tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None,
                                bits(values), cap, over=over, **put)
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


def same_as_mirror(got, want, rows, cap, what):
    recs, over, plies, moves, status = got
    assert np.array_equal(recs, want.records[rows]), what
    assert np.array_equal(over != 0, want.over[rows]) and np.array_equal(plies, want.plies[rows]), what
    assert moves.shape == (len(rows), cap) and not status.any(), what
    width = want.moves.shape[1]                                       # the mirror's history is cut to its longest game
    assert np.array_equal(moves[:, :width], want.moves[rows]) and (moves[:, width:] == NONE).all(), what


# ---- 1. bkt_move_value_playouts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", list(COMBOS))
def test_playouts_equal_the_mirror_byte_for_byte(nine, tables, replies, random_values, combo):
    plain = host_games(nine, tables, combo, np.full((2, 81), 256, np.uint16), "none", replies, RO.MAX_PLIES)
    for form in FORMS:
        for cap in CAPS:
            want = host_games(nine, tables, combo, random_values, form, replies, cap)
            for rows in ([0], [0, 1, 2], [0, 1, 2, 3], list(range(6)), list(range(7)), [8, 3, 5, 0, 7, 2, 6, 1, 4]):
                got = launch(nine, tables, combo, random_values, form, replies, cap, rows=rows)   # seat edges; a permuted order
                same_as_mirror(got, want, np.array(rows), cap, (combo, form, cap, rows))
        assert form != "none" or not np.array_equal(want.moves[:, :8], plain.moves[:, :8])        # the values do enter the draw


def test_playouts_at_the_clamp_and_with_a_learned_table(nine, tables, replies):
    top = (PT.PatternTable(np.full(PT.ENTRIES, 65535, np.uint16)), TC.TacticTable(np.full(TC.ENTRIES, 65535, np.uint16)))
    most = np.full((2, 81), 65535, np.uint16)
    most[0, :20], most[1, 60:] = 100, 256                             # some weights below the clamp: the draw is not uniform
    learned = learned_values().values
    for values, tabs in ((most, top), (np.full((2, 81), 1, np.uint16), tables), (learned, tables)):
        for form in FORMS:
            for cap in (8, RO.MAX_PLIES):
                want = host_games(nine, tabs, "both", values, form, replies, cap)
                same_as_mirror(launch(nine, tabs, "both", values, form, replies, cap), want, np.arange(9), cap, (form, cap))


@pytest.mark.parametrize("combo", list(COMBOS))
def test_neutral_values_play_the_games_of_every_wrapped_entry_point(nine, tables, replies, combo):
    neutral = np.full((2, 81), 256, np.uint16)
    p, t = COMBOS[combo]
    w, tac = tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None
    for cap in CAPS:
        for form in FORMS:
            pos, ctr = dev(nine), dev(RO.default_counters(9, RO.record_turns(nine)))
            if form == "single":
                out = T.reply_playouts(pos, SEED, ctr, w, tac, dev(replies[form]), cap)
            elif form == "pairs":
                out = T.reply2_playouts(pos, SEED, ctr, w, tac, dev(replies[form]), cap)
            elif t:
                out = T.tactical_playouts(pos, SEED, ctr, w, tac, cap)
            elif p:
                out = T.pattern_playouts(pos, SEED, ctr, w, cap)
            else:
                out = T.random_playouts(pos, SEED, ctr, cap)
            sibling = (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)
            for got, sib in zip(launch(nine, tables, combo, neutral, form, replies, cap), sibling):
                assert np.array_equal(got, sib), (combo, form, cap)


def test_a_row_over_on_entry(nine, tables, replies, random_values):
    over = torch.zeros((9,), dtype=torch.uint8, device=DEV)
    over[1] = over[4] = 1
    recs, o, plies, moves, status = launch(nine, tables, "both", random_values, "pairs", replies, RO.MAX_PLIES, over=over)
    assert np.array_equal(recs[[1, 4]], nine[[1, 4]]) and (moves[[1, 4]] == NONE).all() and not plies[[1, 4]].any()
    assert o[1] == 1 and o[4] == 1 and not status.any() and plies[2] > 2
    free = launch(nine, tables, "both", random_values, "pairs", replies, RO.MAX_PLIES)
    keep = [0, 2, 3, 5, 6, 7, 8]                                      # the other rows play the games they play anyway
    assert np.array_equal(recs[keep], free[0][keep]) and np.array_equal(moves[keep], free[3][keep])


def test_refused_playout_calls_write_nothing(nine, replies):
    lib = T.load()
    pos, ctr = dev(nine), dev(RO.default_counters(9, RO.record_turns(nine)))
    over = torch.full((9,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((9,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((9, 8), 77, dtype=torch.int16, device=DEV)
    values = bits(np.full((2, 81), 256, np.uint16))
    single = dev(replies["single"])
    buf = torch.full((13284 + 8,), 255, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0

    def call(p=pos.data_ptr(), batch=9, c=ctr.data_ptr(), v=values.data_ptr(), r1=None, r2=None, cap=8, o=over.data_ptr(),
             n=plies.data_ptr(), s=status.data_ptr()):
        return lib.bkt_move_value_playouts(p, batch, SEED, c, None, None, v, r1, r2, cap, o, n, moves.data_ptr(), s, None)

    for kw in (dict(v=None), dict(r1=single.data_ptr(), r2=buf.data_ptr()), dict(r2=buf.data_ptr() + 1), dict(r2=buf.data_ptr() + 2),
               dict(p=None), dict(c=None), dict(o=None), dict(n=None), dict(s=None), dict(batch=0), dict(batch=T.MAX_BATCH + 1),
               dict(cap=0), dict(cap=1025), dict(r1=single.data_ptr(), cap=0), dict(r2=buf.data_ptr(), batch=-1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), nine) and (over == 7).all().item() and (moves == 77).all().item()
    assert (plies == 77).all().item() and (status == 77).all().item()
    assert call(r2=buf.data_ptr() + 4) == 0                           # 4-byte aligned is enough
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    with pytest.raises(ValueError):
        T.move_value_playouts(pos, SEED, ctr, None, None, values, 8, replies=single, replies2=buf[:13284].view(2, 82, 81))
    with pytest.raises(ValueError):
        T.move_value_playouts(pos, SEED, ctr, None, None, values.view(torch.uint8), 8)
    with pytest.raises(ValueError):
        T.move_value_playouts(pos, SEED, ctr, None, None, values.cpu(), 8)


# ---- 2. bkt_move_value_update ----------------------------------------------------------------------------------------------------
def update(table, recs, moves, won, records, playouts, times=1):
    """T.move_value_update on copies of `table`'s counts and values between guard bytes, with a sentinel-filled scratch and
    guard bytes behind it -> (counts int64 [2,81,2], values uint16 [2,81])."""
    need = T.load().bkt_move_value_scratch_bytes(records)
    assert need == records * 1296
    cbuf = torch.full((32 + 324 + 32,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    vbuf = torch.full((64 + 162 + 64,), 0x5A5A, dtype=torch.int16, device=DEV)
    counts, values = cbuf[32:32 + 324].view(2, 81, 2), vbuf[64:64 + 162].view(2, 81)
    counts.copy_(dev(table.counts))
    values.fill_(0x7777)                                              # every entry is written, whatever stood there
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    lut = bits(table.lut)
    for _ in range(times):
        T.move_value_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, counts, values, lut, table.k,
                            table.limit, scratch)
    assert (cbuf[:32] == 0x5A5A5A5A).all().item() and (cbuf[32 + 324:] == 0x5A5A5A5A).all().item()
    assert (vbuf[:64] == 0x5A5A).all().item() and (vbuf[64 + 162:] == 0x5A5A).all().item()
    assert (scratch[need:] == 0xA5).all().item()
    return counts.cpu().numpy(), values.cpu().numpy().view(np.uint16)


def table_from(seed, k, limit, lut):
    rng = np.random.default_rng(seed)
    counts = np.zeros((2, 81, 2), np.int64)
    counts[..., 0] = rng.integers(0, max(limit, 3000), (2, 81))
    counts[..., 1] = rng.integers(0, 1 << 30, (2, 81)) % (counts[..., 0] + 1)
    counts[0, :5], counts[1, 80] = 0, (1 << 40, 1 << 39)             # never played; far beyond any limit
    return MV.MoveValueTable(counts, np.full((2, 81), lut[32], np.uint16), lut, k, limit)


def same_update(make, recs, moves, won, records, playouts, times=1):
    want = make()
    for _ in range(times):
        plays = MV.move_value_update_host(want, recs, moves, won, records, playouts)
    counts, values = update(make(), recs, moves, won, records, playouts, times)
    assert np.array_equal(counts, want.counts), np.argwhere(counts != want.counts)[:8]
    assert np.array_equal(values, want.values), np.argwhere(values != want.values)[:8]
    return plays


def test_update_equals_the_hand_written_histories():
    for k, limit in ((1, 0), (3, 4), (65536, 16384)):
        assert same_update(lambda: table_from(1, k, limit, ramp_lut()), HAND_RECS, HAND_MOVES, HAND_WON, 2, 4) == 26
        assert same_update(lambda: table_from(1, k, limit, ramp_lut()), np.repeat(HAND_RECS, 4, 0), HAND_MOVES, HAND_WON, 8, 1) == 26


@pytest.fixture(scope="module")
def real(nine):
    """64 uniform playouts of 81 records at the three caps, on the device: histories and winners (the tests take the first
    playouts of a record's 64)."""
    gold = golden_records()
    recs = np.ascontiguousarray(np.concatenate([nine, gold[::max(len(gold) // 72, 1)][:72]]))
    assert len(recs) == 81
    out = {}
    for cap in (1, 8, 400):
        pos = dev(recs).repeat_interleave(64, 0)
        moves = T.random_playouts(pos, SEED, L.value_counters_device(dev(recs), 64), cap)[2]
        won = (T.area_score(pos, L.KOMI) > 0).view(81, 64) == L.black_to_move(dev(recs))[:, None]
        out[cap] = (moves.cpu().numpy(), won.reshape(-1).cpu().numpy().astype(np.uint8))
    return recs, out


@pytest.mark.parametrize("cap", [1, 8, 400])
@pytest.mark.parametrize("records,playouts", [(1, 1), (1, 3), (2, 4), (5, 7), (3, 64), (81, 64)])
def test_update_equals_the_mirror_on_real_histories(real, records, playouts, cap):
    recs, runs = real
    moves, won = runs[cap]
    first = 1 if records < 6 else 0                                   # (record 0 needs no luck: every playout is one move)
    pick = np.arange(first, first + records)
    rows = (pick[:, None] * 64 + np.arange(playouts)[None, :]).reshape(-1)
    lut = MV.lut_of(0.1) if records % 2 else ramp_lut()
    plays = 0
    for k, limit in ((1, 0), (65536, 4), (16, 16384), (1, 16384), (65536, 0)):
        make = lambda: table_from(records * 100 + playouts + k, k, limit, lut)   # noqa: E731  (non-zero counts on entry)
        plays = same_update(make, recs[pick], moves[rows], won[rows], records, playouts)
        assert same_update(lambda: MV.MoveValueTable.empty(0.25, k, limit), recs[pick], moves[rows], won[rows], records, playouts) == plays
    assert plays >= records * playouts // 2 and (cap == 1 or plays > records * playouts)
    first_run, second_run = (update(table_from(3, 16, 16384, lut), recs[pick], moves[rows], won[rows], records, playouts) for _ in range(2))
    assert all(np.array_equal(a, b) for a, b in zip(first_run, second_run))       # two runs are equal


@pytest.mark.parametrize("max_plies", [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024])
def test_update_equals_the_mirror_on_colliding_histories(max_plies):
    for records, playouts, seed in ((3, 5, 40), (1, 9, 70), (13, 1, 71), (40, 2, 72)):   # rounds of four rows, and tails of one to three
        recs, moves, won = random_histories(records, playouts, max_plies, seed + max_plies)
        same_update(lambda: table_from(9, 2, 64, ramp_lut()), recs, moves, won, records, playouts, times=2)


def test_nothing_after_the_end_of_a_row_counts():
    recs, moves, won = random_histories(2, 3, 600, 3, points=9)
    moves[:, :300] = np.random.default_rng(4).integers(0, 9, (6, 300))
    moves[:, 300:520] = NONE                                          # the end, then valid-looking moves from ply 520 on
    moves[:, 520:] = np.random.default_rng(5).integers(0, 9, (6, 80))
    cut = moves.copy()
    cut[:, 300:] = NONE
    want = table_from(5, 1, 0, ramp_lut())
    assert MV.move_value_update_host(want, recs, cut, won, 2, 3) == 6 * 300
    counts, values = update(table_from(5, 1, 0, ramp_lut()), recs, moves, won, 2, 3)
    assert np.array_equal(counts, want.counts) and np.array_equal(values, want.values)


def test_updates_back_to_back_and_the_argument_checks():
    a, b = random_histories(3, 5, 9, 1), random_histories(2, 7, 30, 2)
    want = table_from(4, 2, 32, ramp_lut())
    MV.move_value_update_host(want, *a, 3, 5)
    MV.move_value_update_host(want, *b, 2, 7)
    t = table_from(4, 2, 32, ramp_lut())
    counts, values, lut = dev(t.counts), bits(t.values), bits(t.lut)
    scratch = torch.empty((3 * 1296,), dtype=torch.uint8, device=DEV)  # one scratch for both: the stream orders the launches
    args = [(dev(r), dev(m), dev(w), n, k) for (r, m, w), n, k in ((a, 3, 5), (b, 2, 7))]
    for r, m, w, n, k in args:                                        # queued without a wait in between
        T.move_value_update(r, m, w, n, k, counts, values, lut, 2, 32, scratch)
    assert np.array_equal(counts.cpu().numpy(), want.counts) and np.array_equal(values.cpu().numpy().view(np.uint16), want.values)
    lib = T.load()
    r, m, w, _, _ = args[0]
    cbuf = torch.full((324 + 2,), 0x11, dtype=torch.int64, device=DEV)
    vbuf = torch.full((162,), 0x11, dtype=torch.int16, device=DEV)
    scratch = torch.full((3 * 1296 + 8,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=9, wn=w.data_ptr(), records=3, playouts=5, c=cbuf.data_ptr(), v=vbuf.data_ptr(),
             lu=lut.data_ptr(), k=16, limit=16384, s=scratch.data_ptr()):
        return lib.bkt_move_value_update(p, mv, cap, wn, records, playouts, c, v, lu, k, limit, s, None)

    for kw in (dict(p=None), dict(mv=None), dict(wn=None), dict(c=None), dict(v=None), dict(lu=None), dict(s=None),
               dict(c=cbuf.data_ptr() + 4), dict(s=scratch.data_ptr() + 1), dict(s=scratch.data_ptr() + 2), dict(records=0),
               dict(records=-2), dict(playouts=0), dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1),
               dict(records=1 << 30, playouts=1 << 30), dict(records=1, playouts=1 << 21, cap=1024), dict(cap=0), dict(cap=-8),
               dict(cap=1025), dict(k=0), dict(k=-1), dict(k=65537), dict(limit=1), dict(limit=-1), dict(limit=(1 << 30) + 1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (cbuf == 0x11).all().item() and (vbuf == 0x11).all().item() and (scratch == 0xA5).all().item()
    assert call(c=cbuf.data_ptr() + 8, s=scratch.data_ptr() + 4, k=65536, limit=1 << 30) == 0 and call(k=1, limit=2) == 0
    torch.cuda.synchronize()
    for bad in (dict(scratch=scratch[:100]), dict(k=0), dict(limit=1), dict(counts=counts.view(-1)), dict(values=values.view(torch.uint8)),
                dict(lut=lut[:64]), dict(lut=lut.cpu())):
        kw = {**dict(counts=counts, values=values, lut=lut, k=2, limit=32, scratch=None), **bad}
        with pytest.raises(ValueError):
            T.move_value_update(r, m, w, 3, 5, kw["counts"], kw["values"], kw["lut"], kw["k"], kw["limit"], kw["scratch"])


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
def same_tables(a, b):
    return np.array_equal(a.counts, b.counts) and np.array_equal(a.values, b.values)


def test_the_functions_that_take_a_table_equal_the_host_rules_request_for_request(nine, tables):
    recs = np.ascontiguousarray(nine[[1, 2, 3, 4, 5]])
    for make, kw in ((lambda: None, dict()), (RO.ReplyTable.empty, dict(patterns=tables[0])), (RO.ReplyTable2.empty, dict(patterns=tables[0], tactics=tables[1]))):
        m_dev, m_host = (MV.MoveValueTable.empty(tau=0.1, k=2, limit=64) for _ in range(2))
        r_dev, r_host = make(), make()
        values = []
        for k in range(3):                                            # the table carries from one request to the next
            a, b = (RO.playout_value(recs, 6, SEED + k, rules=rules, replies=r, move_values=m, **kw)
                    for rules, r, m in (("device", r_dev, m_dev), ("host", r_host, m_host)))
            assert np.array_equal(a.view(np.int32), b.view(np.int32)) and same_tables(m_dev, m_host), k
            assert r_dev is None or np.array_equal(r_dev.array, r_host.array), k
            values.append(a)
        assert m_dev.counts[..., 0].max() < 64 and m_dev.occupancy() > 100 and m_dev.values.max() > 256 > m_dev.values.min()
        a, b = (RO.playout_amaf(recs, 6, SEED, rules=rules, replies=r, move_values=m, sides=2, **kw)
                for rules, r, m in (("device", r_dev, m_dev), ("host", r_host, m_host)))
        assert np.array_equal(a.value.view(np.int32), b.value.view(np.int32)) and np.array_equal(a.played, b.played)
        assert np.array_equal(a.won, b.won) and same_tables(m_dev, m_host)
        f_dev, f_host = (RO.random_playouts(recs, SEED, rules=rules, replies=r, move_values=m, **kw)
                         for rules, r, m in (("device", r_dev, m_dev), ("host", r_host, m_host)))
        assert np.array_equal(f_dev.moves[:, :f_host.moves.shape[1]], f_host.moves) and same_tables(m_dev, m_host)
        assert np.array_equal(f_dev.score, f_host.score)
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, replies=RO.ReplyTables(2), slots=np.zeros(5, np.int64), move_values=MV.MoveValueTable.empty())
    with pytest.raises(ValueError, match="move-value"):
        RO.playout_ownership(recs, 2, SEED, move_values=MV.MoveValueTable.empty())


def test_the_evaluator_equals_the_host_rules_and_its_first_request_is_the_plain_one(nine):
    recs = np.ascontiguousarray(nine[[1, 2, 3, 4, 5]])
    same = lambda x: x                                                # noqa: E731
    more = dict(rave=True, replies=2)
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rules=rules, move_values=True, **more) for rules in ("device", "host")]
    plain = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, **more)
    values = []
    for k in range(3):
        d, h = (ev.finish(ev.submit(recs, 2), normalise=same) for ev in evs)
        assert len(d) == len(h) == 3
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert same_tables(evs[0].move_values, evs[1].move_values) and np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        if k == 0:                                                    # a fresh table is neutral: the evaluator without the option
            p = plain.finish(plain.submit(recs, 2), normalise=same)
            assert np.array_equal(d[0].view(np.int32), p[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), p[1].view(np.int32))
            assert all(np.array_equal(x, y) for x, y in zip(d[2][1:], p[2][1:])) and np.array_equal(evs[0].replies.array, plain.replies.array)
        values.append(d[1])
    assert evs[0].move_values.occupancy() > 100
    # two requests in flight see the table in submit order
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, move_values=True, **more)
    h1, h2 = ev.submit(recs, 2), ev.submit(recs, 2)
    assert np.array_equal(ev.finish(h2, normalise=same)[1], values[1]) and np.array_equal(ev.finish(h1, normalise=same)[1], values[0])


def test_native_mcts_with_move_values_is_deterministic_and_equals_the_host_rules():
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][60]   # a mid-game position: shorter playouts
    seen = []
    for rules in ("device", "device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=4, playout_prior=1.0, playout_rave=4, playout_move_values=0.25, playout_seed=SEED,
                       playout_rules=rules, expand_thresh=2)
        assert t.evaluator.rules == rules and type(t.evaluator.move_values) is MV.MoveValueTable and t.evaluator.replies is None
        t.rollout(50)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move, t.evaluator.move_values.counts.copy()))
        t.close()
    for other in seen[1:]:                                            # one seed twice; device rules and host rules
        assert seen[0][0] == other[0] and seen[0][1] == other[1] and np.array_equal(seen[0][2], other[2])
    assert sum(seen[0][0].values()) == 50 and (seen[0][2][..., 0] > 0).sum() > 50

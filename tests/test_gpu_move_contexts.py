"""NAST playouts on the GPU: bkt_move_context_playouts against the host mirror and against every entry point it
must equal byte for byte; bkt_move_context_update against the mirror integer for integer, at the edges of its 64-lane
chunks and of its parameters; the playout kernel on the adversarial boards; and the evaluator and the tree search end to
end."""
import json
import os

import numpy as np
import pytest
import torch

import adversarial_boards as A
from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import movecontexts as MC
from bokego_amd import movevalues as MV
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN
from test_amaf_cpu import seeded_tables
from test_gpu_patterns import _assert_same
from test_mast_cpu import ramp_lut
from test_replies_cpu import random_histories, start
from test_reply_pairs_cpu import NONE, S, learned_nine, nine_records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
CAPS = (1, 5, RO.MAX_PLIES)
BATCHES = (1, 2, 3, 4, 7)                                             # seat edges at three rows a workgroup
SETUPS = {"alone": (True, "none"), "uniform": (False, "none"), "single": (True, "single"), "pairs": (True, "pairs")}
ENTRIES = 2 * 82 * 81
SCRATCH = ENTRIES * 16


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def bits(x):
    return dev(np.array(x, np.uint16).view(np.int16))


@pytest.fixture(scope="module")
def nine():
    return nine_records()


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def replies():
    pairs = learned_nine().array
    return {"none": None, "single": np.ascontiguousarray(pairs[:, S]), "pairs": pairs}


@pytest.fixture(scope="module")
def distinct_values():
    """uint16 [2,82,81], every entry a value of its own over the whole range 1..65535 (37 is coprime to 65535): a wrong
    colour, plane or point index shows."""
    v = ((np.arange(ENTRIES, dtype=np.int64) * 37) % 65535 + 1).astype(np.uint16).reshape(2, 82, 81)
    assert len(np.unique(v)) == ENTRIES and v.min() >= 1
    return v


def table_with(values):
    return MC.MoveContextTable(np.zeros((2, 82, 81, 2), np.int64), values, MV.lut_of(1.0), 1, 0, 1)


def host_games(recs, tables, weighted, values, form, replies, cap):
    table = {"none": None, "single": RO.ReplyTable, "pairs": RO.ReplyTable2}[form]
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(len(recs), RO.record_turns(recs)), len(recs))
    mv = table_with(values) if values.ndim == 3 else MV.MoveValueTable(np.zeros((2, 81, 2), np.int64), values, MV.lut_of(1.0), 1, 0)
    return RO._random_host(recs, key, ctr, cap, L.KOMI, True, tables[0] if weighted else None, tables[1] if weighted else None,
                           None if table is None else table(replies[form]), None, mv)


def launch(recs, tables, weighted, values, form, replies, cap, rows=None, call=None):
    rows = np.arange(len(recs)) if rows is None else np.asarray(rows)
    pos = dev(recs[rows])
    ctr = dev(RO.default_counters(len(recs), RO.record_turns(recs))[rows])
    put = {} if form == "none" else {"replies" if form == "single" else "replies2": dev(replies[form])}
    out = (call or T.move_context_playouts)(pos, SEED, ctr, tables[0].device(DEV) if weighted else None,
                                            tables[1].device(DEV) if weighted else None, bits(values), cap, **put)
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


def same_as_mirror(got, want, rows, cap, what):
    recs, over, plies, moves, status = got
    assert np.array_equal(recs, want.records[rows]), what
    assert np.array_equal(over != 0, want.over[rows]) and np.array_equal(plies, want.plies[rows]), what
    assert moves.shape == (len(rows), cap) and not status.any(), what
    width = want.moves.shape[1]                                       # the mirror's history is cut to its longest game
    assert np.array_equal(moves[:, :width], want.moves[rows]) and (moves[:, width:] == NONE).all(), what


# ---- 1. bkt_move_context_playouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", list(SETUPS))
def test_playouts_equal_the_mirror_byte_for_byte(nine, tables, replies, distinct_values, setup):
    weighted, form = SETUPS[setup]
    recs = np.ascontiguousarray(nine[[3, 1, 2, 4, 5, 7, 8]])          # a mid-game record first: row 0 alone is a real game
    plain = host_games(recs, tables, weighted, np.full((2, 82, 81), 256, np.uint16), form, replies, RO.MAX_PLIES)
    for cap in CAPS:
        want = host_games(recs, tables, weighted, distinct_values, form, replies, cap)
        for batch in BATCHES:
            rows = np.arange(batch)
            same_as_mirror(launch(recs, tables, weighted, distinct_values, form, replies, cap, rows=rows), want, rows, cap, (setup, cap, batch))
    assert not np.array_equal(want.moves, plain.moves)                # the values do enter the draw
    # the plane is the previous move's: with plane 81 everywhere the games are others
    flat = np.ascontiguousarray(np.broadcast_to(distinct_values[:, 81:82], (2, 82, 81)))
    other = host_games(recs, tables, weighted, flat, form, replies, RO.MAX_PLIES)
    assert not np.array_equal(other.moves, want.moves)


@pytest.mark.parametrize("setup", list(SETUPS))
def test_neutral_values_play_the_games_of_every_wrapped_entry_point(nine, tables, replies, setup):
    weighted, form = SETUPS[setup]
    neutral = np.full((2, 82, 81), 256, np.uint16)
    w, tac = (tables[0].device(DEV), tables[1].device(DEV)) if weighted else (None, None)
    for cap in CAPS:
        pos, ctr = dev(nine), dev(RO.default_counters(9, RO.record_turns(nine)))
        if form == "single":
            out = T.reply_playouts(pos, SEED, ctr, w, tac, dev(replies[form]), cap)
        elif form == "pairs":
            out = T.reply2_playouts(pos, SEED, ctr, w, tac, dev(replies[form]), cap)
        elif weighted:
            out = T.tactical_playouts(pos, SEED, ctr, w, tac, cap)
        else:
            out = T.random_playouts(pos, SEED, ctr, cap)
        sibling = (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)
        for got, sib in zip(launch(nine, tables, weighted, neutral, form, replies, cap), sibling):
            assert np.array_equal(got, sib), (setup, cap)


@pytest.mark.parametrize("setup", list(SETUPS))
def test_with_min_plays_at_the_limit_the_games_are_the_move_value_games(nine, tables, replies, setup):
    """A table the device update leaves with min_plays >= limit > 0: every plane is plane 81, and the games are
    bkt_move_value_playouts' on that plane, byte for byte."""
    weighted, form = SETUPS[setup]
    recs, moves, won = random_histories(5, 7, 65, 12, points=81)
    t = MC.MoveContextTable.empty(tau=0.05, k=1, limit=16, min_plays=16)
    counts, values = update(t, recs, moves, won, 5, 7)
    assert (values[:, :81] == values[:, 81:82]).all() and len(np.unique(values[:, 81])) > 8 and counts[:, :81, :, 0].max() < 16
    for cap in (5, RO.MAX_PLIES):
        a = launch(nine, tables, weighted, values, form, replies, cap)
        b = launch(nine, tables, weighted, np.ascontiguousarray(values[:, 81]), form, replies, cap, call=T.move_value_playouts)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (setup, cap)


def test_refused_playout_calls_write_nothing(nine, replies):
    lib = T.load()
    pos, ctr = dev(nine), dev(RO.default_counters(9, RO.record_turns(nine)))
    over = torch.full((9,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((9,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((9, 8), 77, dtype=torch.int16, device=DEV)
    values = bits(np.full((2, 82, 81), 256, np.uint16))
    single = dev(replies["single"])
    buf = torch.full((13284 + 8,), 255, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0

    def call(p=pos.data_ptr(), batch=9, c=ctr.data_ptr(), v=values.data_ptr(), r1=None, r2=None, cap=8, o=over.data_ptr(),
             n=plies.data_ptr(), s=status.data_ptr()):
        return lib.bkt_move_context_playouts(p, batch, SEED, c, None, None, v, r1, r2, cap, o, n, moves.data_ptr(), s, None)

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
        T.move_context_playouts(pos, SEED, ctr, None, None, values, 8, replies=single, replies2=buf[:13284].view(2, 82, 81))
    for bad in (values.view(torch.uint8), values.cpu(), values[:, 81].contiguous()):
        with pytest.raises(ValueError):
            T.move_context_playouts(pos, SEED, ctr, None, None, bad, 8)


# ---- 2. bkt_move_context_update --------------------------------------------------------------------------------------------------
def update(table, recs, moves, won, records, playouts, times=1):
    """T.move_context_update on copies of `table`'s counts and values between guard bands, with a sentinel-filled scratch and
    a guard band behind it -> (counts int64 [2,82,81,2], values uint16 [2,82,81])."""
    assert T.move_context_scratch_bytes(records) == SCRATCH
    cbuf = torch.full((32 + 2 * ENTRIES + 32,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    vbuf = torch.full((64 + ENTRIES + 64,), 0x5A5A, dtype=torch.int16, device=DEV)
    counts, values = cbuf[32:32 + 2 * ENTRIES].view(2, 82, 81, 2), vbuf[64:64 + ENTRIES].view(2, 82, 81)
    counts.copy_(dev(table.counts))
    values.fill_(0x7777)                                              # every entry is written, whatever stood there
    scratch = torch.full((SCRATCH + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    lut = bits(table.lut)
    for _ in range(times):
        T.move_context_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, counts, values, lut, table.k,
                              table.limit, table.min_plays, scratch)
    assert (cbuf[:32] == 0x5A5A5A5A).all().item() and (cbuf[32 + 2 * ENTRIES:] == 0x5A5A5A5A).all().item()
    assert (vbuf[:64] == 0x5A5A).all().item() and (vbuf[64 + ENTRIES:] == 0x5A5A).all().item()
    assert (scratch[SCRATCH:] == 0xA5).all().item()
    return counts.cpu().numpy(), values.cpu().numpy().view(np.uint16)


PARAMS = ((1, 0, 1), (65536, 2, 1), (16, 16384, 8), (16, 16, 16))     # (k, limit, min_plays)


def table_from(seed, k, limit, min_plays, lut):
    """Counts seeded up to four times the limit, some entries never played and one far beyond any limit."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((2, 82, 81, 2), np.int64)
    counts[..., 0] = rng.integers(0, max(4 * limit, 40), (2, 82, 81))
    counts[..., 1] = rng.integers(0, 1 << 30, (2, 82, 81)) % (counts[..., 0] + 1)
    counts[0, :, :5], counts[1, 81, 80], counts[1, 3, 7] = 0, (1 << 40, 1 << 39), (1 << 36, 5)
    return MC.MoveContextTable(counts, np.full((2, 82, 81), lut[32], np.uint16), lut, k, limit, min_plays)


def same_update(make, recs, moves, won, records, playouts, times=2):
    want = make()
    for _ in range(times):
        plays = MC.move_context_update_host(want, recs, moves, won, records, playouts)
    counts, values = update(make(), recs, moves, won, records, playouts, times)
    assert np.array_equal(counts, want.counts), np.argwhere(counts != want.counts)[:8]
    assert np.array_equal(values, want.values), np.argwhere(values != want.values)[:8]
    return plays


@pytest.mark.parametrize("max_plies", [1, 5, 63, 64, 65, 400])
@pytest.mark.parametrize("records,playouts", [(1, 1), (2, 64), (5, 7), (82, 8)])
def test_update_equals_the_mirror(records, playouts, max_plies):
    recs, moves, won = random_histories(records, playouts, max_plies, 100 * records + max_plies)
    moves[0] = np.random.default_rng(max_plies).integers(0, 12, max_plies)        # one row runs the whole width
    plays = 0
    for i, (k, limit, min_plays) in enumerate(PARAMS):
        lut = MV.lut_of(0.1) if i % 2 else ramp_lut()
        plays = same_update(lambda: table_from(records + i, k, limit, min_plays, lut), recs, moves, won, records, playouts)
    assert same_update(lambda: MC.MoveContextTable.empty(), recs, moves, won, records, playouts) == plays
    assert plays >= max_plies


@pytest.mark.parametrize("max_plies", [2, 64, 65, 400])
def test_update_on_colliding_histories_every_row_the_same_two_moves(max_plies):
    """All plays land on two context entries and two plane-81 entries: the sums are exact whatever the order."""
    for records, playouts in ((2, 64), (82, 8)):
        recs = np.stack([start(31, 0)] * records)
        moves = np.tile(np.array([30, 31], np.int16), (records * playouts, max_plies // 2 + 1))[:, :max_plies]
        won = (np.arange(records * playouts) % 3 == 0).astype(np.uint8)
        for k, limit, min_plays in PARAMS:
            plays = same_update(lambda: table_from(7, k, limit, min_plays, ramp_lut()), recs, moves, won, records, playouts)
            assert plays == records * playouts * max_plies
        t = MC.MoveContextTable.empty(k=1, limit=0, min_plays=1)
        counts, _ = update(t, recs, moves, won, records, playouts)
        rows, wins = records * playouts, int(won.sum())
        assert counts[0, 31, 30].tolist() == [rows * ((max_plies + 1) // 2), wins * ((max_plies + 1) // 2)]
        assert counts[1, 30, 31].tolist() == [rows * (max_plies // 2), (rows - wins) * (max_plies // 2)]
        assert np.array_equal(counts[0, 81, 30], counts[0, 31, 30]) and np.array_equal(counts[1, 81, 31], counts[1, 30, 31])
        assert int(counts[..., 0].sum()) == 2 * rows * max_plies


def test_plane_81_is_the_move_value_update_on_the_device():
    for records, playouts, max_plies in ((5, 7, 65), (82, 8, 400)):
        recs, moves, won = random_histories(records, playouts, max_plies, 9)
        for k, limit, min_plays in PARAMS:
            t = table_from(3, k, limit, min_plays, ramp_lut())
            counts, values = update(t, recs, moves, won, records, playouts, times=2)
            c, v, lut = dev(t.counts[:, 81]), bits(np.full((2, 81), 7, np.uint16)), bits(t.lut)
            for _ in range(2):
                T.move_value_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, c, v, lut, k, limit)
            assert np.array_equal(counts[:, 81], c.cpu().numpy()) and np.array_equal(values[:, 81], v.cpu().numpy().view(np.uint16))


def test_updates_back_to_back_and_the_argument_checks():
    a, b = random_histories(3, 5, 9, 1), random_histories(2, 7, 130, 2)
    want = table_from(4, 2, 32, 4, ramp_lut())
    MC.move_context_update_host(want, *a, 3, 5)
    MC.move_context_update_host(want, *b, 2, 7)
    t = table_from(4, 2, 32, 4, ramp_lut())
    counts, values, lut = dev(t.counts), bits(t.values), bits(t.lut)
    scratch = torch.empty((SCRATCH,), dtype=torch.uint8, device=DEV)  # one scratch for both: the stream orders the launches
    args = [(dev(r), dev(m), dev(w), n, k) for (r, m, w), n, k in ((a, 3, 5), (b, 2, 7))]
    for r, m, w, n, k in args:                                        # queued without a wait in between
        T.move_context_update(r, m, w, n, k, counts, values, lut, 2, 32, 4, scratch)
    assert np.array_equal(counts.cpu().numpy(), want.counts) and np.array_equal(values.cpu().numpy().view(np.uint16), want.values)
    lib = T.load()
    r, m, w, _, _ = args[0]
    cbuf = torch.full((2 * ENTRIES + 2,), 0x11, dtype=torch.int64, device=DEV)
    vbuf = torch.full((ENTRIES + 16,), 0x11, dtype=torch.int16, device=DEV)
    scratch = torch.full((SCRATCH + 16,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=9, wn=w.data_ptr(), records=3, playouts=5, c=cbuf.data_ptr(), v=vbuf.data_ptr(),
             lu=lut.data_ptr(), k=16, limit=16384, min_plays=8, s=scratch.data_ptr()):
        return lib.bkt_move_context_update(p, mv, cap, wn, records, playouts, c, v, lu, k, limit, min_plays, s, None)

    for kw in (dict(p=None), dict(mv=None), dict(wn=None), dict(c=None), dict(v=None), dict(lu=None), dict(s=None),
               dict(c=cbuf.data_ptr() + 4), dict(s=scratch.data_ptr() + 1), dict(s=scratch.data_ptr() + 4), dict(records=0),
               dict(records=-2), dict(playouts=0), dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1),
               dict(records=1 << 30, playouts=1 << 30), dict(records=1, playouts=1 << 21, cap=1024), dict(cap=0), dict(cap=-8),
               dict(cap=1025), dict(k=0), dict(k=-1), dict(k=65537), dict(limit=1), dict(limit=-1), dict(limit=(1 << 30) + 1),
               dict(min_plays=0), dict(min_plays=-3), dict(min_plays=(1 << 30) + 1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (cbuf == 0x11).all().item() and (vbuf == 0x11).all().item() and (scratch == 0xA5).all().item()
    assert [T.move_context_scratch_bytes(n) for n in (-1, 0, 1, 82)] == [0, 0, SCRATCH, SCRATCH]
    cbuf.zero_()                                                      # (0 <= won <= played from here on)
    assert call(c=cbuf.data_ptr() + 8, s=scratch.data_ptr() + 8, k=65536, limit=1 << 30, min_plays=1 << 30) == 0
    assert call(k=1, limit=2, min_plays=1) == 0
    torch.cuda.synchronize()
    assert (cbuf[-1] == 0).item() and (vbuf[ENTRIES:] == 0x11).all().item() and (scratch[SCRATCH + 8:] == 0xA5).all().item()
    for bad in (dict(scratch=scratch[:100]), dict(k=0), dict(limit=1), dict(min_plays=0), dict(counts=counts.view(-1)),
                dict(values=values.view(torch.uint8)), dict(values=values[:, 81].contiguous()), dict(lut=lut[:64]), dict(lut=lut.cpu())):
        kw = {**dict(counts=counts, values=values, lut=lut, k=2, limit=32, min_plays=4, scratch=None), **bad}
        with pytest.raises(ValueError):
            T.move_context_update(r, m, w, 3, 5, kw["counts"], kw["values"], kw["lut"], kw["k"], kw["limit"], kw["min_plays"], kw["scratch"])


# ---- 3. the adversarial boards ----------------------------------------------------------------------------------------------------
def test_the_ply_loop_from_the_adversarial_boards(tables, distinct_values):
    """bkt_move_context_playouts reads boards: three playouts of 24 plies from every record of the hand-built corpus against
    the host mirror, whole and in batches of 1 to 4 rows, and the table both calls then learned."""
    recs = A.check_conditions().recs.copy()
    starts = np.repeat(recs, 3, 0)
    kw = dict(patterns=tables[0], tactics=tables[1])
    host_table, dev_table = table_with(distinct_values), table_with(distinct_values)
    host = RO.random_playouts(starts, 11, max_plies=24, rules="host", move_values=host_table, **kw)
    got = RO.random_playouts(starts, 11, max_plies=24, move_values=dev_table, **kw)
    _assert_same(got, host, "move_context")
    assert np.array_equal(dev_table.counts, host_table.counts) and np.array_equal(dev_table.values, host_table.values)
    ctr = RO.default_counters(len(starts), RO.record_turns(starts))
    hard = [3 * A.index(n) for n in ("spiral/w", "ring/b", "arms/b", "cap80_centre/b", "checker/w", "ko_corner/script1")]
    for rows in (1, 2, 3, 4):
        for lo in hard:
            sub = RO.random_playouts(starts[lo:lo + rows], 11, counters=ctr[lo:lo + rows], max_plies=24,
                                     move_values=table_with(distinct_values), **kw)
            assert np.array_equal(sub.records.cpu().numpy(), host.records[lo:lo + rows]), (rows, lo)
            assert np.array_equal(sub.moves, host.moves[lo:lo + rows, :sub.moves.shape[1]]), (rows, lo)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def same_tables(a, b):
    return np.array_equal(a.counts, b.counts) and np.array_equal(a.values, b.values)


@pytest.mark.parametrize("more", [dict(), dict(replies=2)], ids=["alone", "pairs"])
def test_the_evaluator_equals_the_host_rules_and_its_first_request_is_the_plain_one(nine, more):
    recs = np.ascontiguousarray(nine[[1, 2, 3, 4, 5]])
    same = lambda x: x                                                # noqa: E731
    more = dict(rave=True, **more)
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rules=rules, move_contexts=0.25, **more) for rules in ("device", "host")]
    plain = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, **more)
    values = []
    for k in range(3):
        d, h = (ev.finish(ev.submit(recs, 2), normalise=same) for ev in evs)
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert same_tables(evs[0].move_values, evs[1].move_values), k
        assert evs[0].replies is None or np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        if k == 0:                                                    # a fresh table is neutral: the evaluator without the option
            p = plain.finish(plain.submit(recs, 2), normalise=same)
            assert np.array_equal(d[0].view(np.int32), p[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), p[1].view(np.int32))
        values.append(d[1])
    t = evs[0].move_values
    assert type(t) is MC.MoveContextTable and t.occupancy() > 300 and t.qualified() > 0
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, move_contexts=0.25, **more)   # two requests in flight: submit order
    h1, h2 = ev.submit(recs, 2), ev.submit(recs, 2)
    assert np.array_equal(ev.finish(h2, normalise=same)[1], values[1]) and np.array_equal(ev.finish(h1, normalise=same)[1], values[0])


def test_native_mcts_with_move_contexts_is_deterministic_and_equals_the_host_rules():
    r = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][60]   # a mid-game position: shorter playouts
    seen = []
    for rules in ("device", "device", "host"):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=4, playout_prior=1.0, playout_rave=4, playout_move_contexts=0.25, playout_seed=SEED,
                       playout_rules=rules, expand_thresh=2)
        assert t.evaluator.rules == rules and type(t.evaluator.move_values) is MC.MoveContextTable and t.evaluator.replies is None
        t.rollout(50)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move, t.evaluator.move_values.counts.copy()))
        t.close()
    for other in seen[1:]:                                            # one seed twice; device rules and host rules
        assert seen[0][0] == other[0] and seen[0][1] == other[1] and np.array_equal(seen[0][2], other[2])
    assert sum(seen[0][0].values()) == 50 and (seen[0][2][:, :81, :, 0] > 0).sum() > 50

"""A move-value table per game of a self-play batch on the GPU: bkt_move_value_playouts_tables and
bkt_move_value_update_tables against the host mirrors, byte for byte, the identities with the single-table and the
neutral-valued entry points, and the evaluator and self_play end to end."""
import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import movevalues as MV
from bokego_amd import replies as RP
from bokego_amd import rollout as RO
from bokego_amd import selfplay
from test_amaf_cpu import seeded_tables
from test_game_move_values_cpu import learned_tables, same_tables
from test_game_pair_tables_cpu import REQUESTS, abc_tables, nine
from test_game_tables_cpu import KW
from test_mast_cpu import ramp_lut
from test_pattern_prior_cpu import golden_records
from test_replies_cpu import random_histories
from test_reply_pairs_cpu import learned2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
NO = RP.NONE
S = 81
ROWS = 7
SLOTS = np.array([0, 3, 1, -1, 4, 0, 2], np.int32)                    # mixed tables in a workgroup, out of range on either side,
CAPS = (8, RO.MAX_PLIES)                                              # and a last workgroup of one row and two empty seats
COMBOS = {"uniform": (False, False), "patterns": (True, False), "both": (True, True)}
FORMS = ("alone", "singles", "pairs")


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def bits(x):
    return dev(np.array(x, np.uint16).view(np.int16))


@pytest.fixture(scope="module")
def seven():
    return np.ascontiguousarray(nine()[:ROWS])


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def values():
    """uint16 [4,2,81]: the values of four tables learned from three requests, different per game."""
    return learned_tables().values.copy()


@pytest.fixture(scope="module")
def replies():
    """Per form the reply tables of four games: none, single tables [4,2,81], pair tables [4,2,82,81]."""
    pairs = np.concatenate([abc_tables(), np.full((1, 2, 82, 81), NO, np.uint8)])
    singles = np.stack([learned2(nine(), 2, SEED + i)[0].array[:, S] for i in range(4)])
    return {"alone": None, "singles": np.ascontiguousarray(singles), "pairs": pairs}


def tables_of(values):
    t = MV.MoveValueTables(len(values), tau=1.0, k=1, limit=0)
    t.values[...] = values
    return t


def host_games(recs, tables, combo, values, form, replies, slots, cap):
    p, t = COMBOS[combo]
    kind = {"alone": None, "singles": RP.ReplyTables, "pairs": RP.ReplyTables2}[form]
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(len(recs), RO.record_turns(recs)), len(recs))
    return RO._random_host(recs, key, ctr, cap, L.KOMI, True, tables[0] if p else None, tables[1] if t else None,
                           None if kind is None else kind(len(values), replies[form][:len(values)]), slots, tables_of(values))


def weights(tables, combo):
    p, t = COMBOS[combo]
    return (tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None)


def launch(recs, tables, combo, values, form, replies, slots, cap, over=None):
    """T.move_value_playouts with slots on recs -> (records, over, plies, moves, status)."""
    pos, ctr = dev(recs), dev(RO.default_counters(len(recs), RO.record_turns(recs)))
    put = {} if form == "alone" else {"replies" if form == "singles" else "replies2": dev(replies[form][:len(values)])}
    out = T.move_value_playouts(pos, SEED, ctr, *weights(tables, combo), bits(values), cap, over=over, slots=dev(slots), **put)
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


def same_as_mirror(got, want, cap, what):
    recs, over, plies, moves, status = got
    assert np.array_equal(recs, want.records), what
    assert np.array_equal(over != 0, want.over) and np.array_equal(plies, want.plies), what
    assert moves.shape == (len(recs), cap) and not status.any(), what
    width = want.moves.shape[1]                                       # the mirror's history is cut to its longest game
    assert np.array_equal(moves[:, :width], want.moves) and (moves[:, width:] == RO.MOVE_NONE).all(), what


# ---- 1. bkt_move_value_playouts_tables -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("combo", list(COMBOS))
def test_playouts_equal_the_mirror_byte_for_byte(seven, tables, values, replies, combo, form):
    for cap in CAPS:
        want = host_games(seven, tables, combo, values, form, replies, SLOTS, cap)
        same_as_mirror(launch(seven, tables, combo, values, form, replies, SLOTS, cap), want, cap, (combo, form, cap))
    turned = host_games(seven, tables, combo, values, form, replies, (SLOTS + 1) % 4, RO.MAX_PLIES)
    assert not np.array_equal(turned.moves[:, :8], want.moves[:, :8])  # the precondition: other tables, other games


@pytest.mark.parametrize("form", FORMS)
def test_one_table_and_every_slot_zero_is_the_single_table_call(seven, tables, values, replies, form):
    for combo in ("uniform", "both"):
        for cap in CAPS:
            for B in (1, 3, 4, 7):
                pos, ctr = dev(seven[:B]), dev(RO.default_counters(B, RO.record_turns(seven[:B])))
                put = {} if form == "alone" else {"replies" if form == "singles" else "replies2": dev(replies[form][1])}
                sib = T.move_value_playouts(pos, SEED, ctr, *weights(tables, combo), bits(values[1]), cap, **put)
                one = {k: (None if v is None else v[1:2]) for k, v in replies.items()}
                got = launch(seven[:B], tables, combo, values[1:2], form, one, np.zeros(B, np.int32), cap)
                for a, b in zip(got, (pos,) + tuple(sib)):
                    assert np.array_equal(a, b.cpu().numpy()), (form, combo, cap, B)


@pytest.mark.parametrize("combo", list(COMBOS))
def test_neutral_values_play_the_games_of_the_wrapped_entry_points(seven, tables, replies, combo):
    neutral = np.full((4, 2, 81), 256, np.uint16)
    p, t = COMBOS[combo]
    w, tac = weights(tables, combo)
    for cap in CAPS:
        for form in FORMS:
            pos, ctr = dev(seven), dev(RO.default_counters(ROWS, RO.record_turns(seven)))
            if form == "singles":
                out = T.reply_playouts(pos, SEED, ctr, w, tac, dev(replies[form]), cap, slots=dev(SLOTS))
            elif form == "pairs":
                out = T.reply2_playouts(pos, SEED, ctr, w, tac, dev(replies[form]), cap, slots=dev(SLOTS))
            elif t:
                out = T.tactical_playouts(pos, SEED, ctr, w, tac, cap)
            elif p:
                out = T.pattern_playouts(pos, SEED, ctr, w, cap)
            else:
                out = T.random_playouts(pos, SEED, ctr, cap)
            sibling = (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)
            for got, sib in zip(launch(seven, tables, combo, neutral, form, replies, SLOTS, cap), sibling):
                assert np.array_equal(got, sib), (combo, form, cap)


def test_a_row_over_on_entry(seven, tables, values, replies):
    over = torch.zeros((ROWS,), dtype=torch.uint8, device=DEV)
    over[1] = over[4] = 1
    recs, o, plies, moves, status = launch(seven, tables, "both", values, "pairs", replies, SLOTS, RO.MAX_PLIES, over=over)
    assert np.array_equal(recs[[1, 4]], seven[[1, 4]]) and (moves[[1, 4]] == RO.MOVE_NONE).all() and not plies[[1, 4]].any()
    assert o[1] == 1 and o[4] == 1 and not status.any() and plies[2] > 2
    free = launch(seven, tables, "both", values, "pairs", replies, SLOTS, RO.MAX_PLIES)
    keep = [0, 2, 3, 5, 6]                                            # the other rows play the games they play anyway
    assert np.array_equal(recs[keep], free[0][keep]) and np.array_equal(moves[keep], free[3][keep])


def test_every_refused_playout_call_writes_nothing(seven, values, replies):
    lib = T.load()
    pos, ctr = dev(seven), dev(RO.default_counters(ROWS, RO.record_turns(seven)))
    over = torch.full((ROWS,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((ROWS,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((ROWS, 8), 77, dtype=torch.int16, device=DEV)
    v, single, slots = bits(values[:2]), dev(replies["singles"][:2]), dev(np.zeros(ROWS, np.int32))
    buf = torch.full((2 * 13284 + 8,), NO, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0

    def call(p=pos.data_ptr(), batch=ROWS, c=ctr.data_ptr(), val=v.data_ptr(), r1=None, r2=None, count=2, sl=slots.data_ptr(),
             cap=8, o=over.data_ptr(), n=plies.data_ptr(), s=status.data_ptr()):
        return lib.bkt_move_value_playouts_tables(p, batch, SEED, c, None, None, val, r1, r2, count, sl, cap, o, n,
                                                  moves.data_ptr(), s, None)

    for kw in (dict(val=None), dict(r1=single.data_ptr(), r2=buf.data_ptr()), dict(count=0), dict(count=-1),
               dict(count=T.MAX_MOVE_VALUE_TABLES + 1), dict(sl=None), dict(r2=buf.data_ptr() + 1), dict(r2=buf.data_ptr() + 2),
               dict(r2=buf.data_ptr() + 3), dict(p=None), dict(c=None), dict(o=None), dict(n=None), dict(s=None), dict(batch=0),
               dict(batch=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025), dict(r1=single.data_ptr(), cap=0)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), seven) and (over == 7).all().item() and (moves == 77).all().item()
    assert (plies == 77).all().item() and (status == 77).all().item()
    assert call(r2=buf.data_ptr() + 4) == 0                           # 4-byte aligned is enough
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    pairs = dev(replies["pairs"][:2])
    good = dict(values=v, slots=slots)
    for bad in (dict(values=v[0]), dict(slots=slots[:3]), dict(slots=slots.to(torch.int64)), dict(slots=slots.cpu()),
                dict(values=v.cpu()), dict(replies=single, replies2=pairs), dict(replies=dev(replies["singles"][:3])),
                dict(replies2=dev(replies["pairs"][:3])), dict(replies=single[0]), dict(replies2=pairs[0])):
        kw = dict(good, **bad)
        with pytest.raises(ValueError):
            T.move_value_playouts(dev(seven), SEED, ctr, None, None, kw.pop("values"), 8, **kw)


# ---- 2. bkt_move_value_update_tables ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real():
    """8 uniform playouts of 82 records at 400 plies, on the device: histories and winners; records 1 and 2 with 64."""
    gold = golden_records()
    recs = np.ascontiguousarray(np.concatenate([nine(), gold[::max(len(gold) // 73, 1)][:73]]))
    assert len(recs) == 82
    out = {}
    for n, part in ((8, recs), (64, recs[1:3])):
        pos = dev(part).repeat_interleave(n, 0)
        moves = T.random_playouts(pos, SEED, L.value_counters_device(dev(part), n), 400)[2]
        won = (T.area_score(pos, L.KOMI) > 0).view(len(part), n) == L.black_to_move(dev(part))[:, None]
        out[n] = (part, moves.cpu().numpy(), won.reshape(-1).cpu().numpy().astype(np.uint8))
    return out


def some_tables(count, seed, k, limit, lut):
    """`count` tables with counts on entry: played up to max(4 * limit, 3000), so that with a limit the halving runs more than
    once; a few entries never played and one far beyond any limit; values that the update has to overwrite."""
    rng = np.random.default_rng(seed)
    t = MV.MoveValueTables(count, tau=1.0, k=k, limit=limit)
    t.lut = np.array(lut, np.uint16)
    t.counts[..., 0] = rng.integers(0, max(4 * limit, 3000), (count, 2, 81))
    t.counts[..., 1] = rng.integers(0, 1 << 30, (count, 2, 81)) % (t.counts[..., 0] + 1)
    t.counts[:, 0, :5], t.counts[:, 1, 80] = 0, (1 << 40, 1 << 39)
    t.values[...] = rng.integers(1, 65536, (count, 2, 81))
    return t


def update(table, recs, moves, won, records, playouts, slots, times=1):
    """T.move_value_update with slots on copies of `table`'s counts and values between guard tables, with a sentinel-filled
    scratch and guard bytes behind it -> (counts int64 [count,2,81,2], values uint16 [count,2,81])."""
    count = table.count
    need = T.load().bkt_move_value_tables_scratch_bytes(records, count)
    assert need == records * 1296
    cbuf = torch.full((count + 2, 2, 81, 2), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    vbuf = torch.full((count + 2, 2, 81), 0x5A5A, dtype=torch.int16, device=DEV)
    cbuf[1:-1] = dev(table.counts)
    vbuf[1:-1] = bits(table.values)
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    lut = bits(table.lut)
    for _ in range(times):
        T.move_value_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, cbuf[1:-1], vbuf[1:-1], lut, table.k,
                            table.limit, scratch, slots=dev(slots))
    assert (cbuf[0] == 0x5A5A5A5A).all().item() and (cbuf[-1] == 0x5A5A5A5A).all().item()
    assert (vbuf[0] == 0x5A5A).all().item() and (vbuf[-1] == 0x5A5A).all().item() and (scratch[need:] == 0xA5).all().item()
    return cbuf[1:-1].cpu().numpy(), vbuf[1:-1].cpu().numpy().view(np.uint16)


def slot_cases(records, count):
    r = np.arange(records)
    out = (r % count).astype(np.int32)
    out[::2] = np.where(r[::2] % 4 == 0, -1, count)                   # every other record out of range, on both sides
    return [(name, s.astype(np.int32)) for name, s in (("modulo", r % count), ("equal", np.full(records, count - 1)),
                                                        ("descending", (records - 1 - r) % count), ("out", out))]


def same_update(make, recs, moves, won, records, playouts, slots, times=1):
    want, before = make(), make()
    plays = 0
    for _ in range(times):
        plays = MV.move_value_update_host(want, recs, moves, won, records, playouts, slots=slots)
    counts, values = update(before, recs, moves, won, records, playouts, slots, times)
    assert np.array_equal(counts, want.counts), np.argwhere(counts != want.counts)[:8]
    assert np.array_equal(values, want.values), np.argwhere(values != want.values)[:8]
    named = np.isin(np.arange(before.count), slots)                   # a table no record names keeps every byte
    assert np.array_equal(counts[~named], before.counts[~named]) and np.array_equal(values[~named], before.values[~named])
    return plays


@pytest.mark.parametrize("count", [1, 3, 4096])
@pytest.mark.parametrize("records,playouts", [(1, 1), (2, 64), (5, 7), (82, 8)])
def test_update_equals_the_mirror_every_byte_of_every_table(real, records, playouts, count):
    per = 64 if playouts == 64 else 8
    part, moves, won = real[per]
    first = 1 if records == 1 else 0                                  # (record 0 needs no luck: every playout is one move)
    pick = np.arange(first, first + records)
    rows = (pick[:, None] * per + np.arange(playouts)[None, :]).reshape(-1)
    recs, moves, won = part[pick], moves[rows], won[rows]
    plays = 0
    for (k, limit), (name, slots) in zip(((1, 0), (65536, 2), (16, 16384), (1, 16384)), slot_cases(records, count)):
        lut = MV.lut_of(0.1) if limit else ramp_lut()
        make = lambda: some_tables(count, 100 * records + count, k, limit, lut)   # noqa: E731
        plays += same_update(make, recs, moves, won, records, playouts, slots)
    assert plays > records * playouts
    if count == 1:                                                    # tables = 1 and every slot 0: bkt_move_value_update's bytes
        t = some_tables(1, 7, 16, 16384, ramp_lut())
        counts, values, lut = dev(t.counts[0]), bits(t.values[0]), bits(t.lut)
        T.move_value_update(dev(recs), dev(moves), dev(won), records, playouts, counts, values, lut, 16, 16384)
        got = update(t, recs, moves, won, records, playouts, np.zeros(records, np.int32))
        assert np.array_equal(got[0][0], counts.cpu().numpy()) and np.array_equal(got[1][0], values.cpu().numpy().view(np.uint16))


@pytest.mark.parametrize("max_plies", [1, 5, 63, 64, 65, 400])
def test_update_equals_the_mirror_on_colliding_histories(max_plies):
    """Moves on a few points only; the plies pad to 4 entries, and 5, 1 and 7 playouts are no multiple of the 4 staged rows."""
    for records, playouts, count in ((3, 5, 2), (13, 1, 3), (2, 7, 1)):
        recs, moves, won = random_histories(records, playouts, max_plies, 40 + max_plies + records)
        for (k, limit), (name, slots) in zip(((65536, 0), (1, 2), (2, 64), (16, 16384)), slot_cases(records, count)):
            make = lambda: some_tables(count, 9 + records, k, limit, ramp_lut())   # noqa: E731
            same_update(make, recs, moves, won, records, playouts, slots, times=2)


def test_updates_back_to_back_and_the_argument_checks(real):
    part, moves, won = real[8]
    a = (part[:5], moves[:40], won[:40], 5, 8, np.array([2, 0, 2, 1, 2], np.int32))
    b = (part[5:8], moves[40:64], won[40:64], 3, 8, np.array([0, 0, 3], np.int32))
    want = some_tables(3, 9, 2, 32, ramp_lut())
    for recs, m, w, n, k, slots in (a, b):
        MV.move_value_update_host(want, recs, m, w, n, k, slots=slots)
    t = some_tables(3, 9, 2, 32, ramp_lut())
    counts, values, lut = dev(t.counts), bits(t.values), bits(t.lut)
    scratch = torch.empty((5 * 1296,), dtype=torch.uint8, device=DEV)  # one scratch for both: the stream orders the launches
    args = [(dev(recs), dev(m), dev(w), n, k, dev(slots)) for recs, m, w, n, k, slots in (a, b)]
    for recs, m, w, n, k, slots in args:                              # queued without a wait in between
        T.move_value_update(recs, m, w, n, k, counts, values, lut, 2, 32, scratch, slots=slots)
    assert np.array_equal(counts.cpu().numpy(), want.counts) and np.array_equal(values.cpu().numpy().view(np.uint16), want.values)
    lib = T.load()
    r, m, w, _, _, sl = args[0]
    cbuf = torch.full((3 * 324 + 2,), 0x11, dtype=torch.int64, device=DEV)
    vbuf = torch.full((3 * 162,), 0x11, dtype=torch.int16, device=DEV)
    scratch = torch.full((5 * 1296 + 8,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=400, wn=w.data_ptr(), records=5, playouts=8, c=cbuf.data_ptr(), v=vbuf.data_ptr(),
             lu=lut.data_ptr(), k=16, limit=16384, count=3, slots=sl.data_ptr(), s=scratch.data_ptr()):
        return lib.bkt_move_value_update_tables(p, mv, cap, wn, records, playouts, c, v, lu, k, limit, count, slots, s, None)

    for kw in (dict(p=None), dict(mv=None), dict(wn=None), dict(c=None), dict(v=None), dict(lu=None), dict(s=None), dict(slots=None),
               dict(count=0), dict(count=-3), dict(count=T.MAX_MOVE_VALUE_TABLES + 1), dict(c=cbuf.data_ptr() + 4),
               dict(s=scratch.data_ptr() + 1), dict(s=scratch.data_ptr() + 2), dict(records=0), dict(records=-2), dict(playouts=0),
               dict(playouts=-1), dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30),
               dict(records=1, playouts=1 << 21, cap=1024), dict(cap=0), dict(cap=-8), dict(cap=1025), dict(k=0), dict(k=-1),
               dict(k=65537), dict(limit=1), dict(limit=-1), dict(limit=(1 << 30) + 1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (cbuf == 0x11).all().item() and (vbuf == 0x11).all().item() and (scratch == 0xA5).all().item()
    cbuf.fill_(0)                                                     # counts the update can read: 0 <= won <= played
    assert call(c=cbuf.data_ptr() + 8, s=scratch.data_ptr() + 4, k=65536, limit=1 << 30) == 0 and call(k=1, limit=2) == 0
    torch.cuda.synchronize()
    for bad in (dict(scratch=scratch[:100]), dict(k=0), dict(limit=1), dict(counts=counts[0]), dict(values=values[0]),
                dict(values=values.view(torch.uint8)), dict(lut=lut[:64]), dict(slots=sl[:4]), dict(slots=sl.cpu()),
                dict(slots=sl.to(torch.int64)), dict(counts=counts[:2])):
        kw = {**dict(counts=counts, values=values, lut=lut, k=2, limit=32, scratch=None, slots=sl), **bad}
        with pytest.raises(ValueError):
            T.move_value_update(r, m, w, 5, 8, kw["counts"], kw["values"], kw["lut"], kw["k"], kw["limit"], kw["scratch"],
                                slots=kw["slots"])


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("more", [dict(), dict(pair_games=3)])
def test_the_evaluator_equals_the_host_rules_request_for_request(more):
    same = lambda x: x                                                # noqa: E731
    requests = [(nine()[rows], n, np.array(games)) for rows, n, games in REQUESTS]
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rave=True, rules=rules, move_value_games=3, move_value_tau=0.1, **more)
           for rules in ("device", "host")]
    outs = []
    for k, (recs, n, games) in enumerate(requests):
        d, h = (ev.finish(ev.submit(recs, n, games=games), normalise=same) for ev in evs)
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert same_tables(evs[0].move_values, evs[1].move_values), k
        assert not more or np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        outs.append(d)
    assert all(evs[0].move_values.table(g).occupancy() > 50 for g in range(3))
    assert evs[0].move_values.values.max() > 256 > evs[0].move_values.values.min()
    # two requests in flight see the tables in submit order
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rave=True, move_value_games=3, move_value_tau=0.1, **more)
    h1 = ev.submit(*requests[0][:2], games=requests[0][2])
    h2 = ev.submit(*requests[1][:2], games=requests[1][2])
    for h, want in ((h2, outs[1]), (h1, outs[0])):
        got = ev.finish(h, normalise=same)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert all(np.array_equal(x, y) for x, y in zip(got[2][1:], want[2][1:]))
    # the functions that take tables
    recs, slots = requests[0][0], requests[0][2]
    t_dev, t_host = MV.MoveValueTables(3, tau=0.1, k=2, limit=64), MV.MoveValueTables(3, tau=0.1, k=2, limit=64)
    r_dev, r_host = (RO.ReplyTables(3), RO.ReplyTables(3)) if more else (None, None)
    for _ in range(2):
        a, b = (RO.playout_amaf(recs, 6, SEED, rules=rules, replies=r, move_values=t, slots=slots, sides=2)
                for rules, r, t in (("device", r_dev, t_dev), ("host", r_host, t_host)))
        assert np.array_equal(a.value.view(np.int32), b.value.view(np.int32)) and np.array_equal(a.played, b.played)
        assert same_tables(t_dev, t_host) and (r_dev is None or np.array_equal(r_dev.array, r_host.array))
    f_dev, f_host = (RO.random_playouts(recs, SEED, rules=rules, replies=r, move_values=t, slots=slots)
                     for rules, r, t in (("device", r_dev, t_dev), ("host", r_host, t_host)))
    assert np.array_equal(f_dev.moves[:, :f_host.moves.shape[1]], f_host.moves) and same_tables(t_dev, t_host)


def test_self_play_equals_the_host_rules():
    kw = dict(KW, n_games=2, rollouts=12, max_turns=6, rave=4)
    seen = []
    for rules in ("device", "host"):
        ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, move_value_games=2, rules=rules)
        local, _ = selfplay.self_play(ev, **kw)
        assert local["native_loop"] is False and local["dedup"] is False
        seen.append(({g: (v["moves"], local["visits"][g]) for g, v in local["games"].items()}, ev.move_values.copy()))
    assert seen[0][0] == seen[1][0] and same_tables(seen[0][1], seen[1][1])
    assert sorted(seen[0][0]) == [0, 1] and all(seen[0][1].table(g).occupancy() > 50 for g in range(2))

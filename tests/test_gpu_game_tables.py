"""A reply table per game of a self-play batch on the GPU: bkt_reply_playouts_tables and
bkt_reply_update_tables against the host mirror, byte for byte, and the evaluator and self_play end to end."""
import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import replies as RP
from bokego_amd import rollout as RO
from bokego_amd import selfplay
from test_amaf_cpu import seeded_tables
from test_game_tables_cpu import KW, learned_tables, nine_records
from test_gpu_replies import COMBOS, dev, launch
from test_pattern_prior_cpu import golden_records

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
NO = RP.NONE
CAPS = (1, 8, RO.MAX_PLIES)
ROWS = 7


@pytest.fixture(scope="module")
def seven():
    return np.ascontiguousarray(nine_records()[:ROWS])


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def five():
    """Five different learned tables, uint8 [5,2,81]."""
    t = learned_tables(5)
    assert len({x.tobytes() for x in t}) == 5
    return t


def slot_patterns(B, count):
    """different: neighbours differ wherever count allows -- three tables in one workgroup, and a change across every
    workgroup boundary; shared: one table for all; out: the first row -1 and the last row `count`, both out of range."""
    different = (np.arange(B) % count).astype(np.int32)
    out = different.copy()
    out[0], out[-1] = -1, count
    return {"different": different, "shared": np.full(B, count - 1, np.int32), "out": out}


def launch_tables(recs, combo, tables, replies, slots, cap, rows):
    """T.reply_playouts_tables on the first rows of recs -> (records, over, plies, moves, status)."""
    pos = dev(recs[:rows])
    ctr = dev(RO.default_counters(len(recs), RO.record_turns(recs))[:rows])
    p, t = COMBOS[combo]
    out = T.reply_playouts_tables(pos, SEED, ctr, tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None,
                                  dev(replies), dev(slots), cap)
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


# ---- 1. bkt_reply_playouts_tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", list(COMBOS))
def test_playouts_equal_the_mirror_byte_for_byte(seven, tables, five, combo):
    p, t = COMBOS[combo]
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(ROWS, RO.record_turns(seven)), ROWS)
    changed = 0
    for cap in CAPS:
        # a row's game depends on its record, its counters and ITS table alone: the mirror once per table (index 5: all 255),
        # and what a slot pattern must give is row i of the run with table slots[i]
        runs = [RO._random_host(seven, key, ctr, cap, L.KOMI, True, tables[0] if p else None, tables[1] if t else None,
                                RP.ReplyTable(x)) for x in list(five) + [np.full((2, 81), NO, np.uint8)]]
        hist = np.full((6, ROWS, cap), RO.MOVE_NONE, np.int16)
        for k, run in enumerate(runs):
            hist[k, :, :run.moves.shape[1]] = run.moves
        changed += int((hist[:5] != hist[5]).any())
        sibling = launch(seven, combo, tables, None, cap)
        for B in (1, 2, 3, 4, 7):                                     # one seat; a partial workgroup; a full one; full + 1; 2 + 1
            for count in (1, 2, 3, 5):
                for name, slots in slot_patterns(B, count).items():
                    use = np.where((slots >= 0) & (slots < count), slots, 5)
                    recs, over, plies, moves, status = launch_tables(seven, combo, tables, five[:count], slots, cap, B)
                    what = (combo, cap, B, count, name)
                    rows = np.arange(B)
                    assert np.array_equal(recs, np.stack([runs[k].records[i] for i, k in zip(rows, use)])), what
                    assert np.array_equal(over != 0, np.array([runs[k].over[i] for i, k in zip(rows, use)])), what
                    assert np.array_equal(plies, np.array([runs[k].plies[i] for i, k in zip(rows, use)])), what
                    assert moves.shape == (B, cap) and np.array_equal(moves, hist[use, rows]) and not status.any(), what
                # all-255 tables: the sibling launch's bytes, whatever the slots
                got = launch_tables(seven, combo, tables, np.full((count, 2, 81), NO, np.uint8), slot_patterns(B, count)["different"],
                                    cap, B)
                for a, b in zip(got, sibling):
                    assert np.array_equal(a, b[:B]), (combo, cap, B, count)
            # tables = 1: bkt_reply_playouts byte for byte
            for a, b in zip(launch_tables(seven, combo, tables, five[:1], np.zeros(B, np.int32), cap, B),
                            launch(seven, combo, tables, five[0], cap, rows=B)):
                assert np.array_equal(a, b), (combo, cap, B)
    assert changed > 0                                                # the learned tables did change games


def test_every_refused_call_writes_nothing(seven, five):
    lib = T.load()
    pos, ctr = dev(seven), dev(RO.default_counters(ROWS, RO.record_turns(seven)))
    over = torch.full((ROWS,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((ROWS,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((ROWS, 8), 77, dtype=torch.int16, device=DEV)
    replies, slots = dev(five[:2]), dev(np.zeros(ROWS, np.int32))

    def call(p=pos.data_ptr(), batch=ROWS, c=ctr.data_ptr(), r=replies.data_ptr(), count=2, sl=slots.data_ptr(), cap=8,
             o=over.data_ptr(), n=plies.data_ptr(), s=status.data_ptr()):
        return lib.bkt_reply_playouts_tables(p, batch, SEED, c, None, None, r, count, sl, cap, o, n, moves.data_ptr(), s, None)

    for kw in (dict(r=None), dict(sl=None), dict(count=0), dict(count=-1), dict(count=T.MAX_BATCH + 1), dict(p=None), dict(c=None),
               dict(o=None), dict(n=None), dict(s=None), dict(batch=0), dict(batch=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), seven) and (over == 7).all().item() and (moves == 77).all().item()
    assert (plies == 77).all().item() and (status == 77).all().item()
    for bad in (dict(replies=replies[0]), dict(slots=slots[:3]), dict(slots=slots.to(torch.int64)), dict(slots=slots.cpu())):
        with pytest.raises(ValueError):
            T.reply_playouts_tables(pos, SEED, ctr, None, None, **dict(dict(replies=replies, slots=slots), **bad), max_plies=8)


# ---- 2. bkt_reply_update_tables -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real():
    """8 uniform playouts of 82 records at both caps, on the device: histories and winners; records 1 and 2 with 64."""
    gold = golden_records()
    recs = np.ascontiguousarray(np.concatenate([nine_records(), gold[::max(len(gold) // 73, 1)][:73]]))
    assert len(recs) == 82
    out = {}
    for cap in (8, 400):
        for n, part in ((8, recs), (64, recs[1:3])):
            pos = dev(part).repeat_interleave(n, 0)
            moves = T.random_playouts(pos, SEED, L.value_counters_device(dev(part), n), cap)[2]
            won = (T.area_score(pos, L.KOMI) > 0).view(len(part), n) == L.black_to_move(dev(part))[:, None]
            out[cap, n] = (part, moves.cpu().numpy(), won.reshape(-1).cpu().numpy().astype(np.uint8))
    return out


def update(before, recs, moves, won, records, playouts, slots):
    """T.reply_update_tables on tables between guard tables, with a sentinel-filled scratch and guard bytes behind it."""
    count = len(before)
    buf = torch.full((count + 2, 2, 81), 0x5A, dtype=torch.uint8, device=DEV)
    buf[1:-1] = dev(before)
    need = T.load().bkt_reply_scratch_bytes(records)
    assert need == records * 2592
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    T.reply_update_tables(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, buf[1:-1], dev(slots), scratch)
    assert (buf[0] == 0x5A).all().item() and (buf[-1] == 0x5A).all().item() and (scratch[need:] == 0xA5).all().item()
    assert not (scratch[:need] == 0xA5).all().item()
    return buf[1:-1].cpu().numpy()


def some_tables(count, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 81, (count, 2, 81)).astype(np.uint8)
    t[rng.random(t.shape) < 0.3] = NO
    t[:, 1, 40] = 200                                                 # an invalid value in every table
    return t


@pytest.mark.parametrize("cap", [8, 400])
@pytest.mark.parametrize("records,playouts", [(1, 1), (2, 64), (5, 7), (82, 8)])
def test_update_equals_the_mirror_every_byte_of_every_table(real, records, playouts, cap):
    part, moves, won = real[cap, 64 if playouts == 64 else 8]
    per = 64 if playouts == 64 else 8
    first = 1 if records == 1 else 0                                  # (record 0 needs no luck: every playout is one move)
    pick = np.arange(first, first + records)
    rows = (pick[:, None] * per + np.arange(playouts)[None, :]).reshape(-1)
    recs, moves, won = part[pick], moves[rows], won[rows]
    stored = 0
    for count in (1, 3, 82):
        r = np.arange(records)
        out = (r % count).astype(np.int32)
        out[::2] = np.where(r[::2] % 4 == 0, -1, count)               # every other record out of range, on both sides
        for name, slots in (("modulo", r % count), ("equal", np.full(records, count - 1)), ("descending", (records - 1 - r) % count),
                            ("out", out)):
            slots = slots.astype(np.int32)
            before = some_tables(count, 100 * records + count)
            want = before.copy()
            events = RO.reply_update_host(want, recs, moves, won, records, playouts, slots=slots)
            got = update(before, recs, moves, won, records, playouts, slots)
            assert np.array_equal(got, want), (count, name, np.argwhere(got != want)[:5], events)
            named = np.isin(np.arange(count), slots)
            assert np.array_equal(got[~named], before[~named])        # a table no record names keeps every byte
            stored += events[0]
        if count == 1:                                                # tables = 1: bkt_reply_update's bytes
            one = dev(before[0])
            T.reply_update(dev(recs), dev(moves), dev(won), records, playouts, one)
            assert np.array_equal(update(before, recs, moves, won, records, playouts, np.zeros(records, np.int32))[0],
                                  one.cpu().numpy())
    assert stored > 0


def test_two_updates_back_to_back_and_the_argument_checks(real):
    part, moves, won = real[8, 8]
    a = (part[:5], moves[:40], won[:40], 5, 8, np.array([2, 0, 2, 1, 0], np.int32))
    b = (part[5:8], moves[40:64], won[40:64], 3, 8, np.array([0, 0, 2], np.int32))
    before = some_tables(3, 9)
    want = before.copy()
    for recs, m, w, n, k, slots in (a, b):
        RO.reply_update_host(want, recs, m, w, n, k, slots=slots)
    replies = dev(before)
    scratch = torch.empty((5 * 2592,), dtype=torch.uint8, device=DEV)  # one scratch for both: the stream orders the four launches
    args = [(dev(recs), dev(m), dev(w), n, k, dev(slots)) for recs, m, w, n, k, slots in (a, b)]
    for recs, m, w, n, k, slots in args:                              # queued without a wait in between
        T.reply_update_tables(recs, m, w, n, k, replies, slots, scratch)
    assert np.array_equal(replies.cpu().numpy(), want)
    lib = T.load()
    r, m, w, _, _, sl = args[0]
    replies, scratch = dev(before), torch.full((5 * 2592,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=8, wn=w.data_ptr(), records=5, playouts=8, t=replies.data_ptr(), count=3,
             slots=sl.data_ptr(), s=scratch.data_ptr()):
        return lib.bkt_reply_update_tables(p, mv, cap, wn, records, playouts, t, count, slots, s, None)

    for kw in (dict(t=None), dict(slots=None), dict(count=0), dict(count=-3), dict(count=T.MAX_BATCH + 1), dict(p=None),
               dict(mv=None), dict(wn=None), dict(s=None), dict(records=0), dict(records=-2), dict(playouts=0), dict(playouts=-1),
               dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30), dict(cap=0), dict(cap=-8),
               dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(replies.cpu().numpy(), before) and (scratch == 0xA5).all().item()
    with pytest.raises(ValueError):
        T.reply_update_tables(r, m, w, 5, 8, replies, sl, scratch[:100])
    with pytest.raises(ValueError):
        T.reply_update_tables(r, m, w, 5, 8, replies, sl[:4], scratch)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
def test_the_evaluator_equals_the_host_rules_request_for_request():
    nine = nine_records()
    same = lambda x: x                                                # noqa: E731
    requests = [(nine[[1, 3, 4, 5]], 2, np.array([0, 2, 2, 1])), (nine[[3, 1, 4]], 1, np.array([2, 0, 1])),
                (nine[[4, 5, 1, 3]], 2, np.array([1, 1, 0, 2]))]
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rave=True, rules=rules, replies=True, games=3)
           for rules in ("device", "host")]
    outs = []
    for k, (recs, n, games) in enumerate(requests):
        d, h = (ev.finish(ev.submit(recs, n, games=games), normalise=same) for ev in evs)
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        outs.append(d)
    assert (evs[0].replies.occupancy() > 0).all()
    # two requests in flight see the tables in submit order
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rave=True, replies=True, games=3)
    h1 = ev.submit(*requests[0][:2], games=requests[0][2])
    h2 = ev.submit(*requests[1][:2], games=requests[1][2])
    for h, want in ((h2, outs[1]), (h1, outs[0])):
        got = ev.finish(h, normalise=same)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert all(np.array_equal(x, y) for x, y in zip(got[2][1:], want[2][1:]))
    ev.finish(ev.submit(*requests[2][:2], games=requests[2][2]), normalise=same)
    assert np.array_equal(ev.replies.array, evs[1].replies.array)


def test_self_play_equals_the_host_rules():
    kw = dict(KW, n_games=4, rollouts=24, max_turns=10, rave=4)
    seen = []
    for rules in ("device", "host"):
        ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, replies=True, games=4, rules=rules)
        local, _ = selfplay.self_play(ev, **kw)
        assert local["native_loop"] is False and local["dedup"] is False
        seen.append(({g: (v["moves"], local["visits"][g]) for g, v in local["games"].items()}, ev.replies.array.copy()))
    assert seen[0][0] == seen[1][0] and np.array_equal(seen[0][1], seen[1][1])
    assert sorted(seen[0][0]) == [0, 1, 2, 3] and ((seen[0][1] <= 80).sum((1, 2)) > 0).all()

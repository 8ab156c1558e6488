"""A pair reply table per game of a self-play batch on the GPU: bkt_reply2_playouts_tables and
bkt_reply2_update_tables against the host mirror, byte for byte, and the evaluator and self_play end to end."""
import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import replies as RP
from bokego_amd import rollout as RO
from bokego_amd import selfplay
from test_amaf_cpu import seeded_tables
from test_game_pair_tables_cpu import FORCED, REQUESTS, abc_tables, nine
from test_game_tables_cpu import KW
from test_pattern_prior_cpu import golden_records
from test_replies_cpu import random_histories
from test_reply_pairs_cpu import learned2, random_table2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 5
NO = RP.NONE
S = 81
ENTRIES = 13284
SCRATCH = 119556
CAPS = (1, 2, 8, RO.MAX_PLIES)
COMBOS = {"uniform": (False, False), "patterns": (True, False), "tactics": (False, True), "both": (True, True)}
ROWS = 7
KIND = (0, 1, 2, 3, 1)                                                # the five tables of a launch: A, B, C, all 255, B again
EMPTY = 3


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


@pytest.fixture(scope="module")
def seven():
    return np.ascontiguousarray(nine()[:ROWS])


@pytest.fixture(scope="module")
def tables():
    return seeded_tables()


@pytest.fixture(scope="module")
def four():
    """A, B, C (one plane 81, three sets of pair planes) and the all-255 table, uint8 [4,2,82,81]."""
    return np.concatenate([abc_tables(), np.full((1, 2, 82, 81), NO, np.uint8)])


def slot_patterns(B, count):
    """different: neighbours differ wherever count allows -- three tables in one workgroup, and a change across every
    workgroup boundary; shared: one table for all; out: the first row -1 and the last row `count`, both out of range."""
    different = (np.arange(B) % count).astype(np.int32)
    out = different.copy()
    out[0], out[-1] = -1, count
    return {"different": different, "shared": np.full(B, count - 1, np.int32), "out": out}


def launch_tables(recs, combo, tables, replies2, slots, cap, rows, over=None):
    """T.reply2_playouts with slots on the first rows of recs -> (records, over, plies, moves, status)."""
    pos = dev(recs[:rows])
    ctr = dev(RO.default_counters(len(recs), RO.record_turns(recs))[:rows])
    p, t = COMBOS[combo]
    out = T.reply2_playouts(pos, SEED, ctr, tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None,
                            dev(replies2), cap, over=over, slots=dev(slots))
    return (pos.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


def weights(tables, combo):
    p, t = COMBOS[combo]
    return (tables[0].device(DEV) if p else None, tables[1].device(DEV) if t else None)


# ---- 1. bkt_reply2_playouts_tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", list(COMBOS))
def test_playouts_equal_the_mirror_byte_for_byte(seven, tables, four, combo):
    p, t = COMBOS[combo]
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(ROWS, RO.record_turns(seven)), ROWS)
    five = four[list(KIND)]
    for cap in CAPS:
        # a row's game depends on its record, its counters and ITS table alone: the mirror once per table, and what a slot
        # pattern must give is row i of the run with table slots[i] (the all-255 run for a slot out of range)
        runs = [RO._random_host(seven, key, ctr, cap, L.KOMI, True, tables[0] if p else None, tables[1] if t else None,
                                RP.ReplyTable2(x)) for x in four]
        hist = np.full((4, ROWS, cap), RO.MOVE_NONE, np.int16)
        for k, run in enumerate(runs):
            hist[k, :, :run.moves.shape[1]] = run.moves
        if cap == RO.MAX_PLIES and combo == "uniform":                # the precondition: a wrong table would show in every
            free = [i for i in range(ROWS) if i not in FORCED]        # row that has a choice at all
            assert all((hist[a, free] != hist[b, free]).any(1).all() for a, b in ((0, 1), (0, 2), (1, 2), (2, 3)))
        for B in (1, 2, 3, 4, 7):                                     # one seat; a partial workgroup; a full one; full + 1; 2 + 1
            for count in (1, 2, 3, 5):
                for name, slots in slot_patterns(B, count).items():
                    use = np.array([KIND[s] if 0 <= s < count else EMPTY for s in slots])
                    recs, over, plies, moves, status = launch_tables(seven, combo, tables, five[:count], slots, cap, B)
                    what = (combo, cap, B, count, name)
                    rows = np.arange(B)
                    assert np.array_equal(recs, np.stack([runs[k].records[i] for i, k in zip(rows, use)])), what
                    assert np.array_equal(over != 0, np.array([runs[k].over[i] for i, k in zip(rows, use)])), what
                    assert np.array_equal(plies, np.array([runs[k].plies[i] for i, k in zip(rows, use)])), what
                    assert moves.shape == (B, cap) and np.array_equal(moves, hist[use, rows]) and not status.any(), what
            # tables = 1 and every slot 0: bkt_reply2_playouts byte for byte
            pos, c = dev(seven[:B]), dev(RO.default_counters(ROWS, RO.record_turns(seven))[:B])
            sibling = T.reply2_playouts(pos, SEED, c, *weights(tables, combo), dev(four[0]), cap)
            got = launch_tables(seven, combo, tables, four[:1], np.zeros(B, np.int32), cap, B)
            for a, b in zip(got, (pos,) + tuple(sibling)):
                assert np.array_equal(a, b.cpu().numpy()), (combo, cap, B)
    assert sum(r.reply_pair_plies for r in runs) > 0                  # (the last cap, 400: pairs did decide plies)


@pytest.mark.parametrize("combo", ["uniform", "both"])
def test_without_pairs_the_playouts_are_those_of_the_single_move_tables(seven, tables, combo):
    """Planes 0..80 of every table all 255: bkt_reply_playouts_tables on the plane-81s, byte for byte."""
    singles = np.stack([learned2(nine(), 2, SEED + i)[0].array[:, S] for i in range(3)])
    pairs = np.full((3, 2, 82, 81), NO, np.uint8)
    pairs[:, :, S] = singles
    assert len({x.tobytes() for x in singles}) == 3
    for cap in (8, RO.MAX_PLIES):
        for B in (3, 7):
            for name, slots in slot_patterns(B, 3).items():
                got = launch_tables(seven, combo, tables, pairs, slots, cap, B)
                pos, c = dev(seven[:B]), dev(RO.default_counters(ROWS, RO.record_turns(seven))[:B])
                sib = T.reply_playouts_tables(pos, SEED, c, *weights(tables, combo), dev(singles), dev(slots), cap)
                for a, b in zip(got, (pos,) + tuple(sib)):
                    assert np.array_equal(a, b.cpu().numpy()), (combo, cap, B, name)


def test_a_row_over_on_entry(seven, tables, four):
    slots = np.array([0, 1, 2, 0, 1, 2, 0], np.int32)
    over = torch.zeros((ROWS,), dtype=torch.uint8, device=DEV)
    over[1] = over[4] = 1
    recs, o, plies, moves, status = launch_tables(seven, "both", tables, four[:3], slots, RO.MAX_PLIES, ROWS, over=over)
    assert np.array_equal(recs[[1, 4]], seven[[1, 4]]) and (moves[[1, 4]] == RO.MOVE_NONE).all() and not plies[[1, 4]].any()
    assert o[1] == 1 and o[4] == 1 and not status.any() and plies[2] > 2
    free = launch_tables(seven, "both", tables, four[:3], slots, RO.MAX_PLIES, ROWS)
    keep = [0, 2, 3, 5, 6]                                            # the other rows play the games they play anyway
    assert np.array_equal(recs[keep], free[0][keep]) and np.array_equal(moves[keep], free[3][keep])


def test_every_refused_playout_call_writes_nothing(seven, four):
    lib = T.load()
    pos, ctr = dev(seven), dev(RO.default_counters(ROWS, RO.record_turns(seven)))
    over = torch.full((ROWS,), 7, dtype=torch.uint8, device=DEV)
    plies, status = (torch.full((ROWS,), 77, dtype=torch.int32, device=DEV) for _ in range(2))
    moves = torch.full((ROWS, 8), 77, dtype=torch.int16, device=DEV)
    buf = torch.full((2 * ENTRIES + 8,), NO, dtype=torch.uint8, device=DEV)
    slots = dev(np.zeros(ROWS, np.int32))
    assert buf.data_ptr() % 4 == 0

    def call(p=pos.data_ptr(), batch=ROWS, c=ctr.data_ptr(), r=buf.data_ptr(), count=2, sl=slots.data_ptr(), cap=8,
             o=over.data_ptr(), n=plies.data_ptr(), s=status.data_ptr()):
        return lib.bkt_reply2_playouts_tables(p, batch, SEED, c, None, None, r, count, sl, cap, o, n, moves.data_ptr(), s, None)

    for kw in (dict(r=None), dict(r=buf.data_ptr() + 1), dict(r=buf.data_ptr() + 2), dict(r=buf.data_ptr() + 3), dict(sl=None),
               dict(count=0), dict(count=-1), dict(count=T.MAX_REPLY2_TABLES + 1), dict(p=None), dict(c=None), dict(o=None),
               dict(n=None), dict(s=None), dict(batch=0), dict(batch=T.MAX_BATCH + 1), dict(cap=0), dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy(), seven) and (over == 7).all().item() and (moves == 77).all().item()
    assert (plies == 77).all().item() and (status == 77).all().item()
    assert call(r=buf.data_ptr() + 4) == 0                             # 4-byte aligned is enough
    torch.cuda.synchronize()
    assert (status == 0).all().item()
    replies = dev(four[:2])
    for bad in (dict(replies2=replies[0]), dict(replies2=replies[:, :, S].contiguous()), dict(slots=slots[:3]),
                dict(slots=slots.to(torch.int64)), dict(slots=slots.cpu())):
        with pytest.raises(ValueError):
            T.reply2_playouts(dev(seven), SEED, ctr, None, None, **dict(dict(replies2=replies, slots=slots), **bad), max_plies=8)


# ---- 2. bkt_reply2_update_tables ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real():
    """8 uniform playouts of 82 records at both caps, on the device: histories and winners; records 1 and 2 with 64."""
    gold = golden_records()
    recs = np.ascontiguousarray(np.concatenate([nine(), gold[::max(len(gold) // 73, 1)][:73]]))
    assert len(recs) == 82
    out = {}
    for cap in (8, 400):
        for n, part in ((8, recs), (64, recs[1:3])):
            pos = dev(part).repeat_interleave(n, 0)
            moves = T.random_playouts(pos, SEED, L.value_counters_device(dev(part), n), cap)[2]
            won = (T.area_score(pos, L.KOMI) > 0).view(len(part), n) == L.black_to_move(dev(part))[:, None]
            out[cap, n] = (part, moves.cpu().numpy(), won.reshape(-1).cpu().numpy().astype(np.uint8))
    return out


def update(before, recs, moves, won, records, playouts, slots, times=1):
    """T.reply2_update with slots on tables between guard tables, with a sentinel-filled scratch and guard bytes behind it."""
    count = len(before)
    buf = torch.full((count + 2, 2, 82, 81), 0x5A, dtype=torch.uint8, device=DEV)
    buf[1:-1] = dev(before)
    need = T.load().bkt_reply2_tables_scratch_bytes(count)
    assert need == count * SCRATCH
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    assert scratch.data_ptr() % 8 == 0
    for _ in range(times):
        T.reply2_update(dev(recs), dev(moves), dev(won, torch.uint8), records, playouts, buf[1:-1], scratch, slots=dev(slots))
    assert (buf[0] == 0x5A).all().item() and (buf[-1] == 0x5A).all().item() and (scratch[need:] == 0xA5).all().item()
    return buf[1:-1].cpu().numpy()


def some_tables(count, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 81, (count, 2, 82, 81)).astype(np.uint8)      # random tables, so that clears find something
    t[rng.random(t.shape) < 0.3] = NO
    t[:, 1, 40, 40], t[:, 0, S, 3] = 200, 81                          # invalid values in every table
    return t


def slot_cases(records, count):
    r = np.arange(records)
    out = (r % count).astype(np.int32)
    out[::2] = np.where(r[::2] % 4 == 0, -1, count)                   # every other record out of range, on both sides
    return [(name, s.astype(np.int32)) for name, s in (("modulo", r % count), ("equal", np.full(records, count - 1)),
                                                        ("descending", (records - 1 - r) % count), ("out", out))]


@pytest.mark.parametrize("cap", [8, 400])
@pytest.mark.parametrize("records,playouts", [(1, 1), (2, 64), (5, 7), (82, 8)])
def test_update_equals_the_mirror_every_byte_of_every_table(real, records, playouts, cap):
    per = 64 if playouts == 64 else 8
    part, moves, won = real[cap, per]
    first = 1 if records == 1 else 0                                  # (record 0 needs no luck: every playout is one move)
    pick = np.arange(first, first + records)
    rows = (pick[:, None] * per + np.arange(playouts)[None, :]).reshape(-1)
    recs, moves, won = part[pick], moves[rows], won[rows]
    stored = 0
    for count in (1, 3, 82):
        before = some_tables(count, 100 * records + count)
        for name, slots in slot_cases(records, count):
            want = before.copy()
            events = RO.reply2_update_host(want, recs, moves, won, records, playouts, slots=slots)
            got = update(before, recs, moves, won, records, playouts, slots)
            assert np.array_equal(got, want), (count, name, np.argwhere(got != want)[:5], events)
            named = np.isin(np.arange(count), slots)
            assert np.array_equal(got[~named], before[~named])        # a table no record names keeps every byte
            stored += events[0]
            if name == "modulo":                                      # plane 81 is what bkt_reply_update_tables leaves
                singles = dev(before[:, :, S])
                T.reply_update_tables(dev(recs), dev(moves), dev(won), records, playouts, singles, dev(slots))
                assert np.array_equal(got[:, :, S], singles.cpu().numpy()), count
        if count == 1:                                                # tables = 1: bkt_reply2_update's bytes
            one = dev(before[0])
            T.reply2_update(dev(recs), dev(moves), dev(won), records, playouts, one)
            assert np.array_equal(update(before, recs, moves, won, records, playouts, np.zeros(records, np.int32))[0],
                                  one.cpu().numpy())
    assert stored > 0


@pytest.mark.parametrize("max_plies", [63, 64, 65])
def test_update_equals_the_mirror_on_colliding_histories(max_plies):
    """Moves on a few points only, so that many events meet in one entry; 63, 64 and 65 plies are the edges of a wave's chunk."""
    for records, playouts, count in ((3, 5, 2), (13, 1, 3), (1, 5, 1)):
        recs, moves, won = random_histories(records, playouts, max_plies, 40 + max_plies + records)
        before = np.stack([random_table2(9 + i) for i in range(count)])
        for name, slots in slot_cases(records, count):
            want = before.copy()
            RO.reply2_update_host(want, recs, moves, won, records, playouts, slots=slots)
            got = update(before, recs, moves, won, records, playouts, slots)
            assert np.array_equal(got, want), (max_plies, records, name, np.argwhere(got != want)[:8])


def test_updates_back_to_back_twice_and_the_argument_checks(real):
    part, moves, won = real[8, 8]
    a = (part[:5], moves[:40], won[:40], 5, 8, np.array([2, 0, 2, 1, 0], np.int32))
    b = (part[5:8], moves[40:64], won[40:64], 3, 8, np.array([0, 0, 2], np.int32))
    before = some_tables(3, 9)
    want = before.copy()
    for recs, m, w, n, k, slots in (a, b):
        RO.reply2_update_host(want, recs, m, w, n, k, slots=slots)
    replies = dev(before)
    scratch = torch.empty((3 * SCRATCH,), dtype=torch.uint8, device=DEV)   # one scratch for both: the stream orders the launches
    args = [(dev(recs), dev(m), dev(w), n, k, dev(slots)) for recs, m, w, n, k, slots in (a, b)]
    for recs, m, w, n, k, slots in args:                              # queued without a wait in between
        T.reply2_update(recs, m, w, n, k, replies, scratch, slots=slots)
    assert np.array_equal(replies.cpu().numpy(), want)
    again = dev(before)                                               # ... and with the scratch the binding keeps
    for recs, m, w, n, k, slots in args:
        T.reply2_update(recs, m, w, n, k, again, slots=slots)
    assert np.array_equal(again.cpu().numpy(), want)
    # the same update twice from the same start: the same bytes; and applied twice, the fold of the records twice over
    first, second = (update(before, *b) for _ in range(2))
    assert np.array_equal(first, second)
    twice = before.copy()
    for _ in range(2):
        RO.reply2_update_host(twice, *b[:5], slots=b[5])
    assert np.array_equal(update(before, *b, times=2), twice)
    lib = T.load()
    r, m, w, _, _, sl = args[0]
    buf = torch.full((3 * ENTRIES + 8,), 0x11, dtype=torch.uint8, device=DEV)
    scratch = torch.full((3 * SCRATCH + 8,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(p=r.data_ptr(), mv=m.data_ptr(), cap=8, wn=w.data_ptr(), records=5, playouts=8, t=buf.data_ptr(), count=3,
             slots=sl.data_ptr(), s=scratch.data_ptr()):
        return lib.bkt_reply2_update_tables(p, mv, cap, wn, records, playouts, t, count, slots, s, None)

    for kw in (dict(t=None), dict(t=buf.data_ptr() + 1), dict(t=buf.data_ptr() + 2), dict(slots=None), dict(count=0), dict(count=-3),
               dict(count=T.MAX_REPLY2_TABLES + 1), dict(p=None), dict(mv=None), dict(wn=None), dict(s=None),
               dict(s=scratch.data_ptr() + 4), dict(records=0), dict(records=-2), dict(playouts=0), dict(playouts=-1),
               dict(records=1 << 12, playouts=(1 << 12) + 1), dict(records=1 << 30, playouts=1 << 30), dict(cap=0), dict(cap=-8),
               dict(cap=1025)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (buf == 0x11).all().item() and (scratch == 0xA5).all().item()
    with pytest.raises(ValueError):
        T.reply2_update(r, m, w, 5, 8, replies, scratch[:100], slots=sl)
    with pytest.raises(ValueError):
        T.reply2_update(r, m, w, 5, 8, replies, slots=sl[:4])
    with pytest.raises(ValueError):
        T.reply2_update(r, m, w, 5, 8, replies[0], slots=sl)


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------
def test_the_evaluator_equals_the_host_rules_request_for_request():
    same = lambda x: x                                                # noqa: E731
    requests = [(nine()[rows], n, np.array(games)) for rows, n, games in REQUESTS]
    evs = [RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rave=True, rules=rules, pair_games=3) for rules in ("device", "host")]
    outs = []
    for k, (recs, n, games) in enumerate(requests):
        d, h = (ev.finish(ev.submit(recs, n, games=games), normalise=same) for ev in evs)
        assert np.array_equal(d[0].view(np.int32), h[0].view(np.int32)) and np.array_equal(d[1].view(np.int32), h[1].view(np.int32)), k
        assert d[2][0] == h[2][0] and all(np.array_equal(x, y) for x, y in zip(d[2][1:], h[2][1:])), k
        assert np.array_equal(evs[0].replies.array, evs[1].replies.array), k
        outs.append(d)
    assert (evs[0].replies.pairs_occupancy() > 0).all()
    # two requests in flight see the tables in submit order
    ev = RO.PlayoutEvaluator(None, 8, seed=SEED, prior=1.0, rave=True, pair_games=3)
    h1 = ev.submit(*requests[0][:2], games=requests[0][2])
    h2 = ev.submit(*requests[1][:2], games=requests[1][2])
    for h, want in ((h2, outs[1]), (h1, outs[0])):
        got = ev.finish(h, normalise=same)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert all(np.array_equal(x, y) for x, y in zip(got[2][1:], want[2][1:]))
    ev.finish(ev.submit(*requests[2][:2], games=requests[2][2]), normalise=same)
    assert np.array_equal(ev.replies.array, evs[1].replies.array)
    # the functions that take tables
    recs, slots = requests[0][0], requests[0][2]
    t_dev, t_host = RO.ReplyTables2(3), RO.ReplyTables2(3)
    for _ in range(2):
        a, b = (RO.playout_amaf(recs, 6, SEED, rules=rules, replies=t, slots=slots, sides=2)
                for rules, t in (("device", t_dev), ("host", t_host)))
        assert np.array_equal(a.value.view(np.int32), b.value.view(np.int32)) and np.array_equal(a.played, b.played)
        assert np.array_equal(t_dev.array, t_host.array)
    f_dev, f_host = (RO.random_playouts(recs, SEED, rules=rules, replies=t, slots=slots) for rules, t in (("device", t_dev), ("host", t_host)))
    assert np.array_equal(f_dev.moves, f_host.moves) and np.array_equal(t_dev.array, t_host.array)
    assert f_dev.reply_pair_plies is None and f_host.reply_pair_plies > 0


def test_self_play_equals_the_host_rules():
    kw = dict(KW, n_games=4, rollouts=24, max_turns=10, rave=4)
    seen = []
    for rules in ("device", "host"):
        ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, pair_games=4, rules=rules)
        local, _ = selfplay.self_play(ev, **kw)
        assert local["native_loop"] is False and local["dedup"] is False
        seen.append(({g: (v["moves"], local["visits"][g]) for g, v in local["games"].items()}, ev.replies.array.copy()))
    assert seen[0][0] == seen[1][0] and np.array_equal(seen[0][1], seen[1][1])
    assert sorted(seen[0][0]) == [0, 1, 2, 3] and ((seen[0][1][:, :, :S] <= 80).sum((1, 2, 3)) > 0).all()

"""A pair reply table per game of a self-play batch, without a GPU: the host mirror over many pair tables against
the single-table mirror per slot, the precondition that makes a slot mix-up visible, the evaluator with pair_games=,
self_play on the host rules, the flag, and what the header, the bindings and the build say."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import replies as RP
from bokego_amd import rollout as RO
from bokego_amd import selfplay
from bokego_amd.playout_options import PlayoutOptions
from conftest import REPO
from test_game_tables_cpu import KW, _bits
from test_reply_pairs_cpu import learned2, nine_records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
SEED = 5
NO = RP.NONE
S = 81
ENTRIES = 2 * 82 * 81
FORCED = (0, 6)          # records of nine_records() with one possible game: a single move and two passes; two passes

_CACHE = {}


def nine():
    if "nine" not in _CACHE:
        _CACHE["nine"] = nine_records()
    return _CACHE["nine"]


def abc_tables():
    """Three pair tables with the SAME plane 81 and different pair planes, uint8 [3,2,82,81], computed once: A learned from
    four uniform playouts of each of the nine records with seed 5; B the pair planes of the same with seed 6 under A's plane
    81; C no pair at all under A's plane 81.  A row that is handed another's table plays another game only through the
    pair planes: what a mix-up of the slots has to show by."""
    if "abc" not in _CACHE:
        a = learned2(nine(), 4, 5)[0].array.copy()
        b = learned2(nine(), 4, 6)[0].array.copy()
        c = np.full_like(a, NO)
        b[:, S] = c[:, S] = a[:, S]
        _CACHE["abc"] = np.stack([a, b, c])
    return _CACHE["abc"].copy()


def host_counters(recs):
    return L.seed_u64(SEED), L.counters_to_host(RO.default_counters(len(recs), RO.record_turns(recs)), len(recs))


def padded(fin, cap):
    """A Finished's history as the device writes it: [rows, cap], MOVE_NONE behind the longest game."""
    out = np.full((len(fin.moves), cap), RO.MOVE_NONE, np.int16)
    out[:, :fin.moves.shape[1]] = fin.moves
    return out


def histories(recs, n, seed=SEED):
    fin = RO.random_playouts(np.repeat(recs, n, 0), seed, counters=RO.value_counters(recs, n), rules="host")
    return fin.moves, ((fin.score > 0) == np.repeat(L.black_to_move(recs), n)).astype(np.uint8)


# ---- 1. the mirror against the single-table mirror, per slot ----------------------------------------------------------------
SLOTS = np.array([0, 1, 2, 0, 0, 2, 1, 2, 0])                         # table 3 of four is named by no row


def test_a_slot_mix_up_would_show_the_precondition_on_the_mirror_itself():
    """Seed 5, default counters, max_plies 400, the uniform draw: the pair planes of A, B and C decide 22, 24 and 0 plies,
    and the histories differ between any two of the three tables for every record that has more than one possible game --
    records 0 and 6 are forced (one move and two passes; two passes), so no table can change them.  At max_plies 8 only
    records 4 and 5 differ, which is why the comparisons meant to catch a wrong table run at 400."""
    tables = abc_tables()
    assert np.array_equal(tables[0, :, S], tables[1, :, S]) and np.array_equal(tables[0, :, S], tables[2, :, S])
    assert (tables[2, :, :S] == NO).all() and not np.array_equal(tables[0], tables[1])
    key, ctr = host_counters(nine())
    runs = {cap: [RO._random_host(nine(), key, ctr, cap, L.KOMI, True, replies=RP.ReplyTable2(t)) for t in tables]
            for cap in (8, 400)}
    assert [r.reply_pair_plies for r in runs[400]] == [22, 24, 0]
    free = [i for i in range(9) if i not in FORCED]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        differ = (padded(runs[400][a], 400) != padded(runs[400][b], 400)).any(1)
        assert differ[free].all() and not differ[list(FORCED)].any(), (a, b, differ)
    short = np.zeros(9, bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        short |= (padded(runs[8][a], 8) != padded(runs[8][b], 8)).any(1)
    assert np.nonzero(short)[0].tolist() == [4, 5]


def test_tables_and_slots_equal_the_single_table_mirror_per_slot():
    tables = np.concatenate([abc_tables(), abc_tables()[:1]])
    tables[3, 1, 7, 7] = tables[3, 0, S, 3] = 200                     # planted: table 3 is touched by nobody
    key, ctr = host_counters(nine())
    fin = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, replies=RP.ReplyTables2(4, tables), slots=SLOTS)
    pair = single = 0
    for s in range(3):
        rows = np.nonzero(SLOTS == s)[0]
        one = RO._random_host(nine()[rows], key, ctr[rows], 400, L.KOMI, True, replies=RP.ReplyTable2(tables[s]))
        assert np.array_equal(fin.records[rows], one.records) and np.array_equal(fin.plies[rows], one.plies), s
        assert np.array_equal(fin.over[rows], one.over) and np.array_equal(padded(fin, 400)[rows], padded(one, 400)), s
        pair, single = pair + one.reply_pair_plies, single + one.reply_plies
    assert (fin.reply_pair_plies, fin.reply_plies) == (pair, single) and pair > 0
    # a wrong table would show: the same rows under a rotated assignment are other games
    turned = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, replies=RP.ReplyTables2(4, tables), slots=(SLOTS + 1) % 3)
    assert all((padded(fin, 400)[i] != padded(turned, 400)[i]).any() for i in range(9) if i not in FORCED)
    # the update: all 13,284 bytes of every table
    moves, won = histories(nine(), 2)
    got = RP.ReplyTables2(4, tables)
    events = RO.reply2_update_host(got, nine(), moves, won, 9, 2, slots=SLOTS)
    total = np.zeros(3, np.int64)
    for s in range(3):
        rows = np.nonzero(SLOTS == s)[0]
        want = tables[s].copy()
        pick = (rows[:, None] * 2 + np.arange(2)[None, :]).reshape(-1)
        total += RO.reply2_update_host(want, nine()[rows], moves[pick], won[pick], len(rows), 2)
        assert got.array[s].size == ENTRIES and np.array_equal(got.array[s], want) and not np.array_equal(want, tables[s]), s
    assert tuple(total) == events and np.array_equal(got.array[3], tables[3])
    assert got.array[3, 1, 7, 7] == 200 == got.array[3, 0, S, 3]
    # raw arrays are taken as the classes are
    raw = tables.copy()
    assert RO.reply2_update_host(raw, nine(), moves, won, 9, 2, slots=SLOTS) == events and np.array_equal(raw, got.array)


def test_slots_out_of_range_play_as_an_empty_table_and_update_nothing():
    tables = abc_tables()[:2]
    key, ctr = host_counters(nine())
    out = np.array([-1, 2, -1, 2, 1 << 20, -(1 << 20), 2, -1, 2])    # -1, count and +-2^20
    fin = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, replies=RP.ReplyTables2(2, tables), slots=out)
    plain = RO._random_host(nine(), key, ctr, 400, L.KOMI, True)
    assert fin.reply_plies == 0 == fin.reply_pair_plies
    assert np.array_equal(fin.moves, plain.moves) and np.array_equal(fin.records, plain.records)
    moves, won = histories(nine(), 2)
    got = RP.ReplyTables2(2, tables)
    assert RO.reply2_update_host(got, nine(), moves, won, 9, 2, slots=out) == (0, 0, 0) and np.array_equal(got.array, tables)
    mixed = np.where(np.arange(9) % 2 == 0, 1, out)                   # the rows in range still learn
    RO.reply2_update_host(got, nine(), moves, won, 9, 2, slots=mixed)
    assert np.array_equal(got.array[0], tables[0]) and not np.array_equal(got.array[1], tables[1])


def test_one_table_with_all_slots_zero_is_the_single_pair_table_bit_for_bit():
    recs = nine()[[1, 3, 5]]
    one, many = RO.ReplyTable2.empty(), RO.ReplyTables2(1)
    for batch in range(2):
        a = RO.playout_amaf(recs, 3, SEED, rules="host", sides=2, replies=one)
        b = RO.playout_amaf(recs, 3, SEED, rules="host", sides=2, replies=many, slots=np.zeros(3, np.int64))
        for name in ("value", "wins", "played", "won"):
            assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), (batch, name)
        assert np.array_equal(many.array[0], one.array), batch
    assert one.pairs_occupancy() > 0 and many.pairs_occupancy().tolist() == [one.pairs_occupancy()]
    assert many.occupancy().tolist() == [one.occupancy()]
    f1 = RO.random_playouts(recs, SEED, rules="host", replies=one)
    f2 = RO.random_playouts(recs, SEED, rules="host", replies=many, slots=[0, 0, 0])
    assert np.array_equal(f1.moves, f2.moves) and np.array_equal(many.array[0], one.array)
    assert (f1.reply_plies, f1.reply_pair_plies) == (f2.reply_plies, f2.reply_pair_plies) and f2.reply_pair_plies is not None
    assert np.array_equal(RO.playout_value(recs, 2, SEED, rules="host", replies=one),
                          RO.playout_value(recs, 2, SEED, rules="host", replies=many, slots=np.zeros(3, np.int32)))


def test_without_pairs_the_tables_are_the_single_move_tables():
    """Planes 0..80 all 255: the playouts are those of a ReplyTables on the plane-81s, and plane 81 of every table is
    folded as reply_update_host folds those."""
    tables = abc_tables()
    singles = np.full_like(tables, NO)
    singles[:, :, S] = np.stack([learned2(nine(), 2, SEED + i)[0].array[:, S] for i in range(3)])
    assert len({x.tobytes() for x in singles}) == 3
    key, ctr = host_counters(nine())
    slots = np.arange(9) % 3
    a = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, replies=RP.ReplyTables2(3, singles), slots=slots)
    b = RO._random_host(nine(), key, ctr, 400, L.KOMI, True, replies=RP.ReplyTables(3, singles[:, :, S]), slots=slots)
    assert np.array_equal(a.moves, b.moves) and np.array_equal(a.records, b.records)
    assert a.reply_plies == b.reply_plies > 0 and a.reply_pair_plies == 0
    moves, won = histories(nine(), 2)
    pairs, ones = RP.ReplyTables2(3, tables), RP.ReplyTables(3, tables[:, :, S])
    RO.reply2_update_host(pairs, nine(), moves, won, 9, 2, slots=slots)
    RO.reply_update_host(ones, nine(), moves, won, 9, 2, slots=slots)
    assert np.array_equal(pairs.array[:, :, S], ones.array) and np.array_equal(pairs.singles().array, ones.array)


def test_the_tables_class_and_what_is_refused():
    t = RP.ReplyTables2(3)
    assert t.count == 3 and t.array.shape == (3, 2, 82, 81) and t.array.dtype == np.uint8 and (t.array == NO).all()
    assert t.occupancy().tolist() == [0, 0, 0] == t.pairs_occupancy().tolist()
    assert isinstance(t, RP.ReplyTable) and not isinstance(t, (RP.ReplyTable2, RP.ReplyTables))
    assert RO.ReplyTables2 is RP.ReplyTables2 and "ReplyTables2" in RP.__all__ and "ReplyTables2" in RO.__all__
    t.array[1, 0, 4, 5], t.array[1, 1, S, 6], t.array[2, 0, S, 0] = 7, 8, 200
    assert t.occupancy().tolist() == [0, 2, 0] and t.pairs_occupancy().tolist() == [0, 1, 0]
    one = t.table(1)
    assert type(one) is RP.ReplyTable2 and one.array[0, 4, 5] == 7 and one.pairs_occupancy() == 1
    one.array[0, 4, 5] = 9                                            # a copy
    singles = t.singles()
    assert type(singles) is RP.ReplyTables and singles.count == 3 and singles.array[1, 1, 6] == 8 and singles.array[2, 0, 0] == 200
    singles.array[1, 1, 6] = 9
    assert t.array[1, 0, 4, 5] == 7 and t.array[1, 1, S, 6] == 8 and t.copy().array[1, 0, 4, 5] == 7 and t.copy().count == 3
    import copy
    import pickle
    for other in (copy.deepcopy(t), pickle.loads(pickle.dumps(t))):
        assert type(other) is RP.ReplyTables2 and other.count == 3 and np.array_equal(other.array, t.array)
    t.clear()
    assert (t.array == NO).all()
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError):
            RP.ReplyTables2(bad)
    assert RP.ReplyTables2(4096).count == 4096 == T.MAX_REPLY2_TABLES
    with pytest.raises(ValueError):
        RP.ReplyTables2(2, np.zeros((3, 2, 82, 81), np.uint8))
    with pytest.raises(ValueError):
        RP.ReplyTables2(2, np.zeros((2, 2, 81), np.uint8))
    recs = nine()[:3]
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", replies=RP.ReplyTables2(2))
    with pytest.raises(TypeError, match="slots"):                    # a single pair table still refuses them
        RO.playout_value(recs, 2, SEED, rules="host", replies=RP.ReplyTable2.empty(), slots=[0, 0, 0])
    with pytest.raises(TypeError, match="slots"):
        RP.reply2_update_host(RP.ReplyTable2.empty(), recs, *histories(recs, 1), 3, 1, slots=[0, 0, 0])
    for bad in ([0, 0], [0.0, 0.0, 0.0], [[0, 0, 0]]):
        with pytest.raises(ValueError, match="slots"):
            RO.playout_value(recs, 2, SEED, rules="host", replies=RP.ReplyTables2(2), slots=bad)
    assert RP.slots_of(RP.ReplyTables2(2), [1, 0], 2).tolist() == [1, 0] and RP.slots_of(RP.ReplyTable2.empty(), None, 2) is None


# ---- 2. the evaluator ---------------------------------------------------------------------------------------------------------
REQUESTS = [([1, 3, 4, 5], 2, [0, 2, 2, 1]), ([3, 1, 4], 1, [2, 0, 1]), ([4, 5, 1, 3], 2, [1, 1, 0, 2])]


def requests():
    return [(nine()[rows], n, np.array(games)) for rows, n, games in REQUESTS]


def test_the_evaluator_with_a_pair_table_per_game():
    same = lambda x: x                                                # noqa: E731
    base = dict(seed=4, prior=1.0, rave=True, rules="host")
    runs = []
    for _ in range(2):
        ev = RO.PlayoutEvaluator(None, 4, pair_games=3, **base)
        assert ev.wants_games is True and type(ev.replies) is RO.ReplyTables2 and ev.replies.count == 3
        runs.append([_bits(ev.finish(ev.submit(r, n, games=g), normalise=same)) for r, n, g in requests()] + [ev.replies.array.copy()])
    assert runs[0][:3] == runs[1][:3] and np.array_equal(runs[0][3], runs[1][3])      # the same bits when run twice
    assert (ev.replies.occupancy() > 0).all() and (ev.replies.pairs_occupancy() > 0).all()
    with pytest.raises(TypeError, match="games"):
        ev.submit(requests()[0][0], 2)
    ev.reset_replies()
    assert ev.replies.occupancy().tolist() == [0, 0, 0]
    # a game's table is that game's rows evaluated alone, in their own order, through PlayoutEvaluator(replies=2)
    for game in range(3):
        alone = RO.PlayoutEvaluator(None, 4, replies=2, **base)
        for r, n, g in requests():
            rows = np.nonzero(g == game)[0]
            alone.finish(alone.submit(r[rows], 0), normalise=same)
        assert np.array_equal(alone.replies.array, runs[0][3][game]), game
    # not the single-move tables' values
    singles = RO.PlayoutEvaluator(None, 4, replies=True, games=3, **base)
    other = [_bits(singles.finish(singles.submit(r, n, games=g), normalise=same)) for r, n, g in requests()]
    assert other != runs[0][:3]
    # what is refused, and what stays what it is
    for kw in (dict(replies=True), dict(replies=2), dict(games=3), dict(replies=True, games=3)):
        with pytest.raises(TypeError, match="pair_games"):
            RO.PlayoutEvaluator(None, 4, pair_games=3, **dict(base, **kw))
    with pytest.raises(TypeError, match="per game"):
        RO.PlayoutEvaluator(None, 4, replies=2, games=3, **base)
    with pytest.raises(ValueError):
        RO.PlayoutEvaluator(None, 4, pair_games=4097, **base)
    import inspect
    assert list(inspect.signature(RO.PlayoutEvaluator.__init__).parameters)[-3:] == ["replies", "games", "pair_games"]
    assert inspect.signature(RO.PlayoutEvaluator.__init__).parameters["pair_games"].default is None
    for kw, kind, wants in ((dict(replies=2), RO.ReplyTable2, False), (dict(replies=True), RO.ReplyTable, False),
                            (dict(replies=True, games=3), RO.ReplyTables, True), (dict(pair_games=None), type(None), False)):
        ev = RO.PlayoutEvaluator(None, 4, **dict(base, **kw))
        assert type(ev.replies) is kind and ev.wants_games is wants, kw


# ---- 3. self_play ---------------------------------------------------------------------------------------------------------------
def _evaluator(**kw):
    return RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, pair_games=3, rules="host", **kw)


def _play(ev=None, **kw):
    ev = _evaluator() if ev is None else ev
    local, _ = selfplay.self_play(ev, **dict(KW, rave=4, **kw))
    assert local["native_loop"] is False and local["dedup"] is False
    return {g: (v["moves"], local["visits"][g]) for g, v in local["games"].items()}, ev


@pytest.fixture(scope="module")
def played():
    ev = _evaluator()
    ev.replies.array[...] = 7                                         # self_play clears the tables first
    return _play(ev)


def test_self_play_gives_every_game_its_own_pair_table(played):
    games, ev = played
    assert sorted(games) == [0, 1, 2] and all(len(m) > 0 and len(v) == len(m) for m, v in games.values())
    assert (ev.replies.occupancy() > 0).all() and (ev.replies.pairs_occupancy() > 0).all()
    for g in range(3):                                                # a game is a pure function of seed_base + gid; its table
        alone, ev1 = _play(gids=[g])                                  # is the one a fresh evaluator learns: the 7s were cleared
        assert alone == {g: games[g]}, g
        assert np.array_equal(ev1.replies.array[0], ev.replies.array[g]) and ev1.replies.occupancy()[1:].tolist() == [0, 0]
    for kw in (dict(n_pools=2, threads=3), dict(pool_sizes=[2, 1])):  # against the fixture's one pool on one thread
        assert _play(**kw)[0] == games, kw
    singles, _ = _play(RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, replies=True, games=3, rules="host"))
    assert singles != games                                           # not the games of the single-move tables
    with pytest.raises(ValueError, match="reply tables"):             # two tables, three games
        selfplay.self_play(RO.PlayoutEvaluator(None, 8, prior=1.0, pair_games=2, rules="host"), **KW)
    with pytest.raises(ValueError, match="native_loop"):
        _play(native_loop=True)
    with pytest.raises(ValueError, match="dedup"):
        _play(dedup=True)


def test_a_one_game_pool_equals_the_pair_evaluator_driven_by_hand(played):
    games, _ = played
    g = 2
    ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, replies=2, rules="host")       # DESIGN 26's: one table, no games=
    prm = selfplay.search_params(rollouts=16, expand_thresh=2, noise_weight=0.25, sample_plies=2, max_turns=6, prune=1,
                                 record_visits=1, eager_top=2, speculate=0, speculate_rows=8, leaves=1, leaves_visit_only=0)
    pool = selfplay.GamePool([20260 + g], prm, cap=200, threads=1)
    pool.set_task_cap(0)
    pool.set_rave(4)
    while True:
        recs, npol = pool.collect_positions()
        if len(recs) == 0:
            break
        pool.deliver(*ev.finish(ev.submit(recs, npol), normalise=selfplay.normalise_rows))
    moves = pool.moves(0)
    assert (moves, [pool.visits(0, ply) for ply in range(len(moves))]) == games[g]
    pool.close()


# ---- 4. the command line ------------------------------------------------------------------------------------------------------
def test_the_flag_of_selfplay(capsys):
    a = selfplay.parse_args(["--playout-value", "64", "--playout-prior", "1", "--game-rave", "--game-reply-pairs"])
    assert a.game_reply_pairs is True and a.game_replies is False and a.game_rave == 4.0 and a.playout.playout_value == 64
    assert a.playout.playout_reply_pairs is False and a.playout.playout_replies is False
    assert selfplay.game_table_keywords(a, 5) == dict(pair_games=5)
    a = selfplay.parse_args(["--playout-value", "8", "--game-replies", "--game-reply-pairs"])     # pairs contain singles
    assert a.game_reply_pairs is True and a.game_replies is True and selfplay.game_table_keywords(a, 2) == dict(pair_games=2)
    a = selfplay.parse_args(["--playout-value", "8", "--game-replies"])
    assert a.game_reply_pairs is False and selfplay.game_table_keywords(a, 2) == dict(replies=True, games=2)
    a = selfplay.parse_args([])
    assert a.game_reply_pairs is False and selfplay.game_table_keywords(a, 2) == {}
    with pytest.raises(SystemExit):
        selfplay.parse_args(["--game-reply-pairs"])
    err = capsys.readouterr().err
    assert "--game-reply-pairs" in err and "--playout-value" in err
    for flag in ("--playout-rave", "--playout-replies", "--playout-reply-pairs"):       # still not selfplay's
        with pytest.raises(SystemExit):
            selfplay.parse_args(["--playout-value", "8", "--playout-prior", "1", flag])
        assert flag in capsys.readouterr().err
    import argparse
    ap = argparse.ArgumentParser()
    PlayoutOptions.add_arguments(ap, rave=False, replies=False)
    assert "--game-reply-pairs" in " ".join(ap.format_help().split())
    ap = argparse.ArgumentParser()
    PlayoutOptions.add_arguments(ap)
    assert "--game-reply-pairs" not in ap.format_help()
    assert "--game-reply-pairs" in selfplay.self_play.__doc__ or "pair_games" in selfplay.self_play.__doc__
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "--game-rave --game-reply-pairs" in readme


# ---- 5. header, bindings, build -----------------------------------------------------------------------------------------------
OLD_KERNELS = ("reply_playouts_kernel", "reply_uniform_playouts_kernel", "reply_summaries_kernel", "reply_apply_kernel",
               "random_playouts_kernel", "pattern_playouts_kernel", "tactical_playouts_kernel", "codes_kernel",
               "lgr2_playouts_kernel", "lgr2_uniform_playouts_kernel", "lgr2_init_kernel", "lgr2_store_kernel",
               "lgr2_clear_kernel", "lgr2_finish_kernel")


def kernels_of(name):
    return re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)+(\w+)\s*\(", open(os.path.join(CSRC, name)).read())


def test_header_bindings_makefile_and_the_kernels_names():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    assert re.search(r"#define\s+BKT_MAX_REPLY2_TABLES\s+4096\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_reply2_playouts_tables\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*const\s+uint8_t\s*\*\s*replies2\s*,\s*int\s+tables\s*,"
                     r"\s*const\s+int32_t\s*\*\s*slots\s*,\s*int\s+max_plies\s*,\s*uint8_t\s*\*\s*over\s*,"
                     r"\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,\s*int32_t\s*\*\s*status\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bsize_t\s+bkt_reply2_tables_scratch_bytes\s*\(\s*int\s+tables\s*\)", code)
    assert re.search(r"\bint\s+bkt_reply2_update_tables\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*const\s+int16_t\s*\*\s*moves\s*,"
                     r"\s*int\s+max_plies\s*,\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*uint8_t\s*\*\s*replies2\s*,\s*int\s+tables\s*,\s*const\s+int32_t\s*\*\s*slots\s*,"
                     r"\s*void\s*\*\s*scratch\s*,\s*void\s*\*\s*stream\s*\)", code)
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("replies2 is uint8 [tables][2][82][81] on the device, 4-byte aligned",
                   "A slot outside 0..tables-1 is compared before it indexes anything",
                   "such a row plays as if its table were all 255, and such a record updates no table",
                   "1 <= tables <= BKT_MAX_REPLY2_TABLES", "it is bkt_reply2_playouts byte for byte",
                   "bkt_reply_playouts_tables on the plane-81s byte for byte", "a table that no record names keeps every byte",
                   "tables * 119556 bytes on the device, 8-byte aligned", "the pair planes stay in global memory",
                   "A refused call launches nothing and writes nothing"):
        assert " ".join(phrase.replace("*", " ").split()) in flat, phrase
    P, I, U64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t
    assert T.SYMBOLS["bkt_reply2_playouts_tables"] == (I, [P, I, U64, P, P, P, P, I, P, I, P, P, P, P, P])
    assert T.SYMBOLS["bkt_reply2_tables_scratch_bytes"] == (Z, [I])
    assert T.SYMBOLS["bkt_reply2_update_tables"] == (I, [P, P, I, P, I, I, P, I, P, P, P])
    import inspect
    for f in (T.reply2_playouts, T.reply2_update):
        assert inspect.signature(f).parameters["slots"].default is None
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        lib.bkt_reply2_tables_scratch_bytes.restype, lib.bkt_reply2_tables_scratch_bytes.argtypes = Z, [I]
        assert lib.bkt_abi_version() == 4 and lib.bkt_reply2_playouts_tables and lib.bkt_reply2_update_tables
        assert [lib.bkt_reply2_tables_scratch_bytes(n) for n in (-1, 0, 1, 3, 4096, 4097)] == \
            [0, 0, 119556, 3 * 119556, 4096 * 119556, 0]
    # the Makefile: a dependency of the library's rule, not a source on its compile line
    make = open(os.path.join(CSRC, "Makefile")).read()
    rule, line = re.search(r"^\$\(TRAIN_OUT\):(.*)\n\t(.*)$", make, flags=re.M).groups()
    assert "bk_playout_reply2_tables.hip" in rule.split() and "bk_playout_reply2_tables.hip" not in line
    # included as text at the very end of bk_playout_pat.hip, after bk_playout_reply2.hip
    includes = re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, "bk_playout_pat.hip")).read(), flags=re.M)
    assert includes[-2:] == ["bk_playout_reply2.hip", "bk_playout_reply2_tables.hip"]
    # the kernels: names that no test's substring picks up, and the siblings' files as they were
    new = kernels_of("bk_playout_reply2_tables.hip")
    assert len(new) == 6 and len(set(new)) == 6 and all(k.startswith("gamepairs_") for k in new), new
    assert not [(k, old) for k in new for old in OLD_KERNELS if old in k]
    assert len(kernels_of("bk_playout_reply2.hip")) == 6 and len(kernels_of("bk_playout_reply.hip")) == 7
    own = open(os.path.join(CSRC, "bk_playout_reply2_tables.hip")).read()
    assert "float" not in own and "double" not in own and own.count("lgr2_events(") == 2 and "__syncthreads" not in own
    assert "GamePairsDraw<WeightedDraw<OptionalTacticalWeight>>" in own and "GamePairsDraw<TrackedUniformDraw>" in own


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_new_kernels_keep_the_resource_conditions_beside_the_kernels_they_wrap(tmp_path):
    """Zero spills and zero scratch in every kernel of the translation unit; the two playout kernels at an occupancy of at
    least the tactical kernel's, itself at least 4, within 128 VGPRs, and with at most 16 bytes of LDS more than the
    kernels of DESIGN 25 they are the siblings of."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(spills) == 2 * len(blocks) and len(scratch) == len(blocks)
    assert all(int(n) == 0 for _, n in spills) and all(int(n) == 0 for n in scratch), (spills, scratch)

    def fields(name):
        (block,) = [b for b in blocks if re.search(r"\d" + name + "E", b.split()[0])]
        return {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in
                (("occupancy", r"Occupancy \[waves/SIMD\]"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                 ("sspill", r"SGPRs Spill"), ("vspill", r"VGPRs Spill"), ("lds", r"LDS Size \[bytes/block\]"),
                 ("vgprs", r" VGPRs"))}

    tactical = fields("tactical_playouts_kernel")
    for new, sibling in (("gamepairs_weighted_kernel", "reply_tables_playouts_kernel"),
                         ("gamepairs_uniform_kernel", "reply_tables_uniform_playouts_kernel")):
        f, g = fields(new), fields(sibling)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (new, f)
        assert f["occupancy"] >= tactical["occupancy"] >= 4 and f["vgprs"] <= 128, (new, f, tactical)
        assert f["lds"] <= g["lds"] + 16, (new, f, g)
    for name in ("gamepairs_init_kernel", "gamepairs_store_kernel", "gamepairs_clear_kernel", "gamepairs_finish_kernel"):
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0 and f["occupancy"] >= 8 and f["lds"] == 0, (name, f)

"""A reply table per game of a self-play batch, without a GPU: bk_pool_batch_games, the host mirror over many
tables, the evaluator with games=, self_play with RAVE and per-game tables on the host rules, the two flags, and the build."""
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
from test_amaf_cpu import three_records
from test_pattern_prior_cpu import eyes_only_record, golden_records, ko_record
from test_replies_cpu import learned

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SEED = 5
NO = RP.NONE


def nine_records():
    """The nine records of tests/test_gpu_replies.py."""
    gold = golden_records()
    black = L.black_to_move(gold)
    mid = np.stack([gold[60], gold[61 + int(np.argmax(black[61:] != black[60]))]])
    recs = np.ascontiguousarray(np.concatenate([three_records(), mid, ko_record(), eyes_only_record(), gold[30:32]]))
    assert len(recs) == 9
    return recs


def learned_tables(count, recs=None, seed=SEED):
    """`count` different learned tables: table i from two playouts of three of the nine records, starting at record i."""
    recs = nine_records() if recs is None else recs
    out = np.stack([learned(recs[np.arange(i, i + 3) % 9], 2, seed + i)[0].array for i in range(count)])
    assert ((out <= 80).sum((1, 2)) > 0).all()
    return out


# ---- 1. bk_pool_batch_games ---------------------------------------------------------------------------------------------------
class _Stub:
    """An evaluator of position records: uniform priors, zero values."""
    wants_positions = True

    def __call__(self, recs, n_policy):
        return np.full((n_policy, 81), 1.0 / 81, np.float32), np.zeros(len(recs), np.float32)


def _pool(n=5, **kw):
    prm = selfplay.search_params(rollouts=6, expand_thresh=2, max_turns=4, eager_top=2, **kw)
    return selfplay.GamePool(np.arange(n) + 77, prm, cap=400, threads=1)


def test_batch_games_names_the_game_of_every_row():
    lib, ev = selfplay.treelib(), _Stub()
    pool = _pool()
    games = np.full(400, -7, np.int32)
    assert lib.bk_pool_batch_games(pool._h, games.ctypes.data, 400) == -1 and (games == -7).all()   # before the first collect
    with pytest.raises(RuntimeError):
        pool.batch_games()
    seen, several = set(), 0
    for step in range(12):
        recs, npol = pool.collect_positions() if step % 2 == 0 else pool.collect()      # both collect flavours
        if len(recs) == 0:
            break
        owner = pool.batch_games()
        assert owner.dtype == np.int32 and len(owner) == len(recs) and ((owner >= 0) & (owner < 5)).all()
        if step % 2 == 0:
            for row, g in enumerate(owner):
                assert lib.bk_pool_find(pool._h, int(g), recs[row].ctypes.data) >= 0, (step, row, g)
        seen.update(owner.tolist())
        several += len(set(owner.tolist())) > 1
        if len(recs) > 1:                                             # cap too small: -1, nothing written
            assert lib.bk_pool_batch_games(pool._h, games.ctypes.data, len(recs) - 1) == -1 and (games == -7).all()
        if step % 2 == 0:
            pool.deliver(*ev(recs, npol))
        else:
            pool.deliver(*ev(np.zeros((len(recs), 192), np.uint8), npol))
        assert lib.bk_pool_batch_games(pool._h, games.ctypes.data, 400) == -1 and (games == -7).all()   # after deliver
    assert seen == set(range(5)) and several > 0 and step >= 4
    pool.close()
    pool = _pool()
    pool.set_dedup(True)                                              # a row may belong to several games: refused
    recs, npol = pool.collect_positions()
    assert len(recs) > 0 and lib.bk_pool_batch_games(pool._h, games.ctypes.data, 400) == -1 and (games == -7).all()
    pool.deliver(*ev(recs, npol))
    pool.close()


# ---- 2. the host mirror over many tables ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nine():
    return nine_records()


@pytest.fixture(scope="module")
def histories(nine):
    """Two uniform host playouts of each of the nine records, and who won them."""
    fin = RO.random_playouts(np.repeat(nine, 2, 0), SEED, counters=RO.value_counters(nine, 2), rules="host")
    return fin.moves, ((fin.score > 0) == np.repeat(L.black_to_move(nine), 2)).astype(np.uint8)


SLOTS = np.array([0, 1, 2, 0, 0, 2, 1, 2, 0])                         # three tables of a count of four: table 3 is named by no row


def test_tables_and_slots_equal_the_single_table_mirror_per_slot(nine, histories):
    tables = learned_tables(4, nine)
    tables[3, 1, 7] = 200                                             # planted: table 3 is touched by nobody
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(9, RO.record_turns(nine)), 9)
    fin = RO._random_host(nine, key, ctr, 24, L.KOMI, True, replies=RP.ReplyTables(4, tables), slots=SLOTS)
    decided = 0
    for s in range(3):
        rows = np.nonzero(SLOTS == s)[0]
        one = RO._random_host(nine[rows], key, ctr[rows], 24, L.KOMI, True, replies=RP.ReplyTable(tables[s]))
        assert np.array_equal(fin.records[rows], one.records) and np.array_equal(fin.plies[rows], one.plies), s
        assert np.array_equal(fin.over[rows], one.over), s
        w = one.moves.shape[1]
        assert np.array_equal(fin.moves[rows, :w], one.moves) and (fin.moves[rows, w:] == RO.MOVE_NONE).all(), s
        decided += one.reply_plies
    assert fin.reply_plies == decided > 0
    # the update: all 162 bytes of every table
    moves, won = histories
    got = RP.ReplyTables(4, tables)
    events = RO.reply_update_host(got, nine, moves, won, 9, 2, slots=SLOTS)
    total = np.zeros(3, np.int64)
    for s in range(3):
        rows = np.nonzero(SLOTS == s)[0]
        want = tables[s].copy()
        pick = (rows[:, None] * 2 + np.arange(2)[None, :]).reshape(-1)
        total += RO.reply_update_host(want, nine[rows], moves[pick], won[pick], len(rows), 2)
        assert np.array_equal(got.array[s], want) and not np.array_equal(want, tables[s]), s
    assert tuple(total) == events and np.array_equal(got.array[3], tables[3]) and got.array[3, 1, 7] == 200


def test_slots_out_of_range_play_as_an_empty_table_and_update_nothing(nine, histories):
    tables = learned_tables(2, nine)
    key, ctr = L.seed_u64(SEED), L.counters_to_host(RO.default_counters(9, RO.record_turns(nine)), 9)
    out = np.array([-1, 2, -1, 2, 1 << 20, -(1 << 20), 2, -1, 2])
    fin = RO._random_host(nine, key, ctr, 24, L.KOMI, True, replies=RP.ReplyTables(2, tables), slots=out)
    plain = RO._random_host(nine, key, ctr, 24, L.KOMI, True)
    assert fin.reply_plies == 0 and np.array_equal(fin.moves, plain.moves) and np.array_equal(fin.records, plain.records)
    moves, won = histories
    got = RP.ReplyTables(2, tables)
    assert RO.reply_update_host(got, nine, moves, won, 9, 2, slots=out) == (0, 0, 0) and np.array_equal(got.array, tables)
    mixed = np.where(np.arange(9) % 2 == 0, 1, out)                   # the rows in range still learn
    RO.reply_update_host(got, nine, moves, won, 9, 2, slots=mixed)
    assert np.array_equal(got.array[0], tables[0]) and not np.array_equal(got.array[1], tables[1])


def test_one_table_with_all_slots_zero_is_todays_single_table(nine):
    recs = nine[[1, 3, 5]]
    one, many = RO.ReplyTable.empty(), RO.ReplyTables(1)
    for batch in range(2):
        a = RO.playout_amaf(recs, 3, SEED, rules="host", sides=2, replies=one)
        b = RO.playout_amaf(recs, 3, SEED, rules="host", sides=2, replies=many, slots=np.zeros(3, np.int64))
        for name in ("value", "wins", "played", "won"):
            assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), (batch, name)
        assert np.array_equal(many.array[0], one.array), batch
    assert one.occupancy() > 0 and many.occupancy().tolist() == [one.occupancy()]
    f1, f2 = RO.random_playouts(recs, SEED, rules="host", replies=one), \
        RO.random_playouts(recs, SEED, rules="host", replies=many, slots=[0, 0, 0])
    assert np.array_equal(f1.moves, f2.moves) and f1.reply_plies == f2.reply_plies and np.array_equal(many.array[0], one.array)
    assert np.array_equal(RO.playout_value(recs, 2, SEED, rules="host", replies=one),
                          RO.playout_value(recs, 2, SEED, rules="host", replies=many, slots=np.zeros(3, np.int32)))


def test_the_tables_class_and_what_is_refused(nine):
    t = RP.ReplyTables(3)
    assert t.count == 3 and t.array.shape == (3, 2, 81) and t.array.dtype == np.uint8 and (t.array == NO).all()
    assert t.occupancy().tolist() == [0, 0, 0] and isinstance(t, RP.ReplyTable) and RO.ReplyTables is RP.ReplyTables
    t.array[1, 0, 5] = 7
    one = t.table(1)
    assert type(one) is RP.ReplyTable and one.array[0, 5] == 7 and one.occupancy() == 1 and t.occupancy().tolist() == [0, 1, 0]
    one.array[0, 5] = 9                                               # a copy
    assert t.array[1, 0, 5] == 7 and t.copy().array[1, 0, 5] == 7 and t.copy().count == 3
    t.clear()
    assert (t.array == NO).all()
    for bad in (0, -1, 65537):
        with pytest.raises(ValueError):
            RP.ReplyTables(bad)
    with pytest.raises(ValueError):
        RP.ReplyTables(2, np.zeros((3, 2, 81), np.uint8))
    recs = nine[:3]
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", replies=RP.ReplyTables(2))
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", replies=RP.ReplyTable.empty(), slots=[0, 0, 0])
    with pytest.raises(TypeError, match="slots"):
        RO.playout_value(recs, 2, SEED, rules="host", slots=[0, 0, 0])
    for bad in ([0, 0], [0.0, 0.0, 0.0], [[0, 0, 0]]):
        with pytest.raises(ValueError, match="slots"):
            RO.playout_value(recs, 2, SEED, rules="host", replies=RP.ReplyTables(2), slots=bad)


# ---- 3. the evaluator --------------------------------------------------------------------------------------------------------------
def _bits(out):
    return [np.asarray(x).tobytes() for x in out[:2]] + [np.asarray(x).tobytes() for x in out[2][1:]]


def test_the_evaluator_with_a_table_per_game(nine):
    same = lambda x: x                                                # noqa: E731
    base = dict(seed=4, prior=1.0, rave=True, rules="host")
    requests = [(nine[[1, 3, 4, 5]], 2, np.array([0, 2, 2, 1])), (nine[[3, 1, 4]], 1, np.array([2, 0, 1])),
                (nine[[4, 5, 1, 3]], 2, np.array([1, 1, 0, 2]))]
    runs = []
    for _ in range(2):
        ev = RO.PlayoutEvaluator(None, 4, replies=True, games=3, **base)
        assert ev.wants_games is True and isinstance(ev.replies, RO.ReplyTables) and ev.replies.count == 3
        runs.append([_bits(ev.finish(ev.submit(r, n, games=g), normalise=same)) for r, n, g in requests] + [ev.replies.array.copy()])
    assert runs[0][:3] == runs[1][:3] and np.array_equal(runs[0][3], runs[1][3])
    assert (ev.replies.occupancy() > 0).all()
    with pytest.raises(TypeError, match="games"):
        ev.submit(requests[0][0], 2)
    ev.reset_replies()
    assert ev.replies.occupancy().tolist() == [0, 0, 0]
    # a game's table sees only its own rows: game 1 alone, in its own row order, leaves table 1 as it was in the batch
    alone = RO.PlayoutEvaluator(None, 4, replies=True, games=3, **base)
    for r, n, g in requests:
        rows = np.nonzero(g == 1)[0]
        alone.finish(alone.submit(r[rows], 0, games=g[rows]), normalise=same)
    assert np.array_equal(alone.replies.array[1], runs[0][3][1]) and alone.replies.occupancy()[[0, 2]].tolist() == [0, 0]
    # games=None: today's evaluator, results and handle fields
    old, new = RO.PlayoutEvaluator(None, 4, replies=True, **base), RO.PlayoutEvaluator(None, 4, replies=True, games=None, **base)
    assert old.wants_games is False and new.wants_games is False and type(new.replies) is RO.ReplyTable
    assert RO.PlayoutEvaluator.wants_games is False and "wants_games" not in vars(new)
    for r, n, _ in requests:
        h_old, h_new = old.submit(r, n), new.submit(r, n)
        assert set(vars(h_old)) == set(vars(h_new)) and set(vars(h_old.run)) == set(vars(h_new.run))
        assert _bits(old.finish(h_old, normalise=same)) == _bits(new.finish(h_new, normalise=same))
    assert np.array_equal(old.replies.array, new.replies.array)
    with pytest.raises(TypeError, match="games"):
        new.submit(requests[0][0], 2, games=requests[0][2])
    with pytest.raises(TypeError, match="replies"):
        RO.PlayoutEvaluator(None, 4, games=3, **base)


# ---- 4. self_play ---------------------------------------------------------------------------------------------------------------------
KW = dict(n_games=3, rollouts=16, max_turns=6, record_visits=1, expand_thresh=2, noise_weight=0.25, sample_plies=2, cap=200,
          threads=1, eager_top=2, n_pools=1, task_cap=0, speculate=0)


def _evaluator(**kw):
    return RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, replies=True, games=3, rules="host", **kw)


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


def test_self_play_gives_every_game_its_own_table(played):
    games, ev = played
    assert sorted(games) == [0, 1, 2] and all(len(m) > 0 and len(v) == len(m) for m, v in games.values())
    assert (ev.replies.occupancy() > 0).all()                         # every used table learned something
    seen = []                                                         # the RAVE tables of the roots, step by step

    def roots(steps, pools):
        seen.append(pools[0].node_rave(0, selfplay.treelib().bk_pool_root_id(pools[0]._h, 0)))

    for g in range(3):                                                # a game is a pure function of seed_base + gid
        alone, ev1 = _play(gids=[g], progress=roots)
        assert alone == {g: games[g]}, g
        assert np.array_equal(ev1.replies.array[0], ev.replies.array[g]) and ev1.replies.occupancy()[1:].tolist() == [0, 0]
    assert seen and any(r is not None and r[0].sum() > 0 for r in seen)
    for kw in (dict(n_pools=2, threads=3), dict(pool_sizes=[2, 1])):  # against the fixture's one pool on one thread
        assert _play(**kw)[0] == games, kw
    plain, _ = selfplay.self_play(RO.PlayoutEvaluator(None, 8, prior=1.0, rules="host"), **KW)
    assert {g: (v["moves"], plain["visits"][g]) for g, v in plain["games"].items()} != games


def test_a_one_game_pool_equals_the_single_table_evaluator_driven_by_hand(played):
    games, _ = played
    g = 2
    ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, replies=True, rules="host")     # today's: one table, no games=
    prm = selfplay.search_params(rollouts=16, expand_thresh=2, noise_weight=0.25, sample_plies=2, max_turns=6, prune=1,
                                 record_visits=1, eager_top=2, speculate=0, speculate_rows=8, leaves=1, leaves_visit_only=0)
    pool = selfplay.GamePool([20260 + g], prm, cap=200, threads=1)
    pool.set_task_cap(0)
    pool.set_rave(4)
    while True:
        recs, npol = pool.collect_positions()
        if len(recs) == 0:
            break
        assert (pool.batch_games() == 0).all()
        pool.deliver(*ev.finish(ev.submit(recs, npol), normalise=selfplay.normalise_rows))
    moves = pool.moves(0)
    assert (moves, [pool.visits(0, ply) for ply in range(len(moves))]) == games[g]
    pool.close()


def test_what_self_play_and_the_native_loop_refuse():
    with pytest.raises(ValueError, match="native_loop"):
        _play(native_loop=True)
    with pytest.raises(ValueError, match="dedup"):
        _play(dedup=True)
    with pytest.raises(ValueError, match="native_loop"):              # RAVE alone needs the Python loop too
        selfplay.self_play(RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, rules="host"), **dict(KW, rave=4, native_loop=True))
    with pytest.raises(TypeError, match="rave"):                      # rave=k needs the records
        selfplay.self_play(RO.PlayoutEvaluator(None, 8, prior=1.0, rules="host"), **dict(KW, rave=4))
    with pytest.raises(ValueError, match="reply tables"):             # two tables, three games
        selfplay.self_play(RO.PlayoutEvaluator(None, 8, prior=1.0, replies=True, games=2, rules="host"), **KW)
    pool = _pool(2)
    for ev in (_evaluator(), RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, rules="host")):
        with pytest.raises(TypeError, match="Python"):
            selfplay.callback_evaluator(ev)
        with pytest.raises(TypeError, match="Python"):
            selfplay.run_pools_native([pool], ev)
    pool.close()
    # RAVE alone keeps de-duplication as it is (bk_pool_deliver_rave takes either collect's layout)
    ev = RO.PlayoutEvaluator(None, 8, prior=1.0, rave=True, rules="host")
    small = dict(KW, rave=4, max_turns=2, rollouts=6)
    on, _ = selfplay.self_play(ev, **dict(small, dedup=True))
    off, _ = selfplay.self_play(ev, **dict(small, dedup=False))
    assert on["dedup"] is True and off["dedup"] is False and on["games"] == off["games"] and on["native_loop"] is False


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------
def test_the_two_flags_of_selfplay(capsys):
    a = selfplay.parse_args(["--playout-value", "64", "--playout-prior", "1", "--game-rave", "--game-replies"])
    assert a.game_rave == 4.0 and a.game_replies is True and a.playout.playout_value == 64
    assert a.playout.playout_rave == 0.0 and a.playout.playout_replies is False
    assert selfplay.parse_args(["--playout-value", "8", "--playout-prior", "0.5", "--game-rave", "16"]).game_rave == 16.0
    a = selfplay.parse_args(["--playout-value", "8", "--game-replies"])          # the tables alone need no prior
    assert a.game_replies is True and a.game_rave == 0.0
    a = selfplay.parse_args([])
    assert a.game_rave == 0.0 and a.game_replies is False
    assert not hasattr(a, "playout_rave") and not hasattr(a, "playout_replies")
    for argv, flag, needs in ((["--game-rave"], "--game-rave", "--playout-value"),
                              (["--game-replies"], "--game-replies", "--playout-value"),
                              (["--playout-value", "8", "--game-rave"], "--game-rave", "--playout-prior"),
                              (["--playout-value", "8", "--playout-prior", "1", "--game-rave", "-1"], "--game-rave", "0 or more")):
        with pytest.raises(SystemExit):
            selfplay.parse_args(argv)
        err = capsys.readouterr().err
        assert flag in err and needs in err, (argv, err)
    for flag in ("--playout-rave", "--playout-replies"):              # still not selfplay's
        with pytest.raises(SystemExit):
            selfplay.parse_args(["--playout-value", "8", "--playout-prior", "1", flag])
        assert flag in capsys.readouterr().err
    import argparse
    ap = argparse.ArgumentParser()
    PlayoutOptions.add_arguments(ap, rave=False, replies=False)
    text = " ".join(ap.format_help().split())
    assert "--game-rave" in text and "--game-replies" in text
    ap = argparse.ArgumentParser()
    PlayoutOptions.add_arguments(ap)
    assert "--game-rave" not in ap.format_help()
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "selfplay --playout-value 64 --playout-prior 1 --game-rave --game-replies --out r/" in readme


# ---- 6. header, bindings, build -------------------------------------------------------------------------------------------------
def test_headers_and_bindings_name_the_new_symbols():
    src = open(os.path.join(REPO, "include", "bokego_train.h")).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_reply_playouts_tables\s*\(\s*void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*uint64_t\s+seed\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*counters\s*,\s*const\s+uint16_t\s*\*\s*table\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*tactics\s*,\s*const\s+uint8_t\s*\*\s*replies\s*,\s*int\s+tables\s*,"
                     r"\s*const\s+int32_t\s*\*\s*slots\s*,\s*int\s+max_plies\s*,\s*uint8_t\s*\*\s*over\s*,"
                     r"\s*int32_t\s*\*\s*plies\s*,\s*int16_t\s*\*\s*moves\s*,\s*int32_t\s*\*\s*status\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+bkt_reply_update_tables\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*const\s+int16_t\s*\*\s*moves\s*,"
                     r"\s*int\s+max_plies\s*,\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*uint8_t\s*\*\s*replies\s*,\s*int\s+tables\s*,\s*const\s+int32_t\s*\*\s*slots\s*,"
                     r"\s*void\s*\*\s*scratch\s*,\s*void\s*\*\s*stream\s*\)", code)
    flat = " ".join(src.replace("*", " ").split())
    for phrase in ("replies is uint8 [tables][2][81] on the device", "slots[i] is the table of row i",
                   "A slot outside 0..tables-1 is compared before it indexes anything",
                   "such a row plays as if its table were all 255, and such a record updates no table",
                   "1 <= tables <= BKT_MAX_BATCH", "a table that no record names keeps every byte",
                   "every table is owned by exactly one workgroup", "replies == NULL or slots == NULL returns BKT_ERR_ARG",
                   "Integers only, no atomics, no workgroup waits on another"):
        assert " ".join(phrase.replace("*", " ").split()) in flat, phrase
    P, I, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert T.SYMBOLS["bkt_reply_playouts_tables"] == (I, [P, I, U64, P, P, P, P, I, P, I, P, P, P, P, P])
    assert T.SYMBOLS["bkt_reply_update_tables"] == (I, [P, P, I, P, I, I, P, I, P, P, P])
    assert callable(T.reply_playouts_tables) and callable(T.reply_update_tables)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_reply_playouts_tables and lib.bkt_reply_update_tables
    tree = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bokego_tree.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bk_pool_batch_games\s*\(\s*const\s+bk_pool\s*\*\s*p\s*,\s*int32_t\s*\*\s*games\s*,"
                     r"\s*int\s+cap\s*\)", tree)
    assert selfplay.TREE_SYMBOLS["bk_pool_batch_games"] == (I, [P, P, I]) and selfplay.treelib().bk_pool_batch_games
    own = open(os.path.join(CSRC, "bk_playout_reply.hip")).read()
    assert "atomic" not in own.replace("no atomics", "") and "float" not in own
    # one draw and one apply body serve one table and many
    assert own.count("struct ReplyDraw") == 1 and "ReplyTablesDraw" not in own and "reply_tables_apply_kernel" not in own
    assert own.count("void reply_apply(") == 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_new_kernels_build_without_spills_or_scratch_at_their_siblings_occupancy(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_pat.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]

    def fields(name):
        (block,) = [b for b in blocks if re.search(r"\d" + name + "E", b.split()[0])]
        return {k: int(re.search(pat + r": (\d+)", block).group(1)) for k, pat in
                (("occupancy", r"Occupancy \[waves/SIMD\]"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                 ("sspill", r"SGPRs Spill"), ("vspill", r"VGPRs Spill"), ("lds", r"LDS Size \[bytes/block\]"))}

    for new, old in (("reply_tables_playouts_kernel", "reply_playouts_kernel"),
                     ("reply_tables_uniform_playouts_kernel", "reply_uniform_playouts_kernel")):
        f, g = fields(new), fields(old)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0, (new, f)
        assert f["occupancy"] >= g["occupancy"] >= 4, (new, f, g)
        # two more tables of 162 bytes (+ 2 of padding each), rounded up
        assert f["lds"] <= g["lds"] + 2 * 164 + 8, (new, f, g)
    for name in ("reply_apply_kernel", "reply_slots_apply_kernel"):   # the two instantiations of the one apply body
        f = fields(name)
        assert f["scratch"] == 0 and f["sspill"] == 0 and f["vspill"] == 0 and f["occupancy"] >= 8 and f["lds"] == 0, (name, f)

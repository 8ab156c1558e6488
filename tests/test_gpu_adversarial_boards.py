"""-m gpu: every device entry point that reads a Go board, on the hand-built corpus of adversarial_boards.py --
chains and empty regions that need dozens of flood rounds, captures of 80, 24 and 8 stones, one chain touching the move
four times, kos at the centre, on an edge and in a corner, suicides, sides with one legal point or none, dense boards with
chains that have no liberty, and records whose liberty cache holds stale counts.  Every comparison is with the host rules
(libbkgo, checked against the reference on these records in test_adversarial_boards_cpu.py) or with the Python mirrors of
rollout.py / patterns.py / tactics.py, and every one is exact: bytes and integers, no tolerance anywhere.

No test skips or filters a corpus record.  Where an entry point's contract asks something of its rows, the test says so and
counts the rows it ran."""
import ctypes
import os

import numpy as np
import pytest
import torch

import adversarial_boards as A
from bokego_amd import _trainlib as T
from bokego_amd import go
from bokego_amd import lockstep as L
from bokego_amd import movevalues as MV
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from bokego_amd.bkw import load_bkw
from bokego_amd.engine import LeafEngine
from conftest import GOLDEN
from test_gpu_patterns import _assert_same
from test_gpu_rollout import device_step, host_step

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NONE = RO.MOVE_NONE
SEED, CAP, PLAYOUTS = 11, 24, 3
_PP = ctypes.POINTER(go.Pos)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def corpus():
    C = A.check_conditions()
    assert len(C.recs) >= 500
    return C


@pytest.fixture(scope="module")
def recs(corpus):
    return corpus.recs.copy()


def host_planes(recs):
    """bk_features_batch_u8 of the records (on a copy: it refreshes the cache it reads)."""
    c = np.array(recs, np.uint8, order="C")
    out = np.empty((len(c), 27, 9, 9), np.uint8)
    L.features_batch(c, out.ctypes.data)
    return out


def host_play(recs, moves):
    """bkt_play_moves' contract on the host: bk_pos_play + bk_pos_liberties on the rows whose move is >= 0
    -> (records, status)."""
    out = np.array(recs, np.uint8, order="C")
    status = np.zeros(len(out), np.int32)
    lib, tmp = go.golib(), (ctypes.c_uint8 * 81)()
    play, base = L._play_fn(), out.ctypes.data
    for i, m in enumerate(np.asarray(moves).tolist()):
        if m < 0:
            continue
        status[i] = play(base + 192 * i, m)
        if status[i] == 0:
            lib.bk_pos_liberties(ctypes.cast(base + 192 * i, _PP), tmp)
    return out, status


def same_rows(got, want, what, moves=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} rows differ, first row {bad[0]}" +
                           ("" if moves is None else f" move {moves[bad[0]]}") +
                           f" at {np.nonzero((got[bad[0]] != want[bad[0]]).reshape(-1))[0][:8]}")


def batches(recs):
    """The whole corpus in each of the three seats of a workgroup, then batches of 1, 2, 3 and 4 rows that walk through it:
    -> (row indices, records)."""
    n = len(recs)
    for k in range(3):
        idx = np.roll(np.arange(n), k)
        yield idx, np.ascontiguousarray(recs[idx])
    yield from A.small_batches(recs)


# ---- 1. the encoder ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = LeafEngine(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw")),
                   max_batch=4096)
    yield e
    e.close()


def test_encoder_planes_equal_the_host(eng, corpus, recs):
    """bk_encode_positions reads the liberty cache and does not refresh it (engine.py: "liberty cache refreshed by the
    host"), so every record goes in with bk_pos_liberties applied -- all of them, none left out: the planes are those of
    bk_features_batch_u8 on the record as the corpus holds it."""
    want, fresh = host_planes(recs), A.refreshed(recs)
    rows = calls = 0
    for idx, part in batches(fresh):
        same_rows(eng.encode_positions(part), want[idx], f"encode_positions, {len(idx)} rows from {idx[0]}")
        rows += len(idx)
        calls += 1
    n = len(recs)
    assert rows == 3 * n + sum(-(-n // b) * b for b in (1, 2, 3, 4)) and calls == 3 + sum(-(-n // b) for b in (1, 2, 3, 4))
    f = want[A.index("ring/b")].reshape(27, 81)
    assert f[13:20, 40].tolist() == [0, 0, 0, 4, 0, 0, 0] and f[20:27, 40].tolist() == [0, 0, 0, 0, 0, 0, 7]


@pytest.mark.parametrize("size", [1, 2, 5, 17, 0])
def test_submit_positions_equals_submit_planes(eng, recs, size):
    """The planes the leaf kernel computes while it stages records (requests of up to 1,024): logits, probs and value are
    the bits of the same request made with the host's planes.  size 0: the whole corpus in one request."""
    want, fresh = host_planes(recs), A.refreshed(recs)
    n = len(recs)
    size = size or n
    rows = 0
    for lo in range(0, n, size):
        idx = np.arange(lo, lo + size) % n
        a = eng.wait(eng.submit_positions(fresh[idx], logits=True, probs=True, value=True))
        b = eng.wait(eng.submit(want[idx], logits=True, probs=True, value=True))
        for k in ("logits", "probs", "value"):
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (size, lo, k)
        rows += len(idx)
    assert rows >= n


# ---- 2. bkt_play_moves ---------------------------------------------------------------------------------------------------------
MOVES = np.arange(86, dtype=np.int32)                                    # every point, and 81..85: off the board


def test_play_moves_every_record_at_every_point(recs):
    n = len(recs)
    rows = np.repeat(recs, len(MOVES), 0)
    moves = np.tile(MOVES, n)
    assert len(rows) == 86 * n <= T.MAX_BATCH
    want, want_st = host_play(rows, moves)
    d = dev(rows)
    planes = torch.full((len(rows), 27, 9, 9), 99, dtype=torch.uint8, device=DEV)
    st = T.play_moves(d, dev(moves), planes)
    assert np.array_equal(st.cpu().numpy(), want_st), np.nonzero(st.cpu().numpy() != want_st)[0][:8]
    same_rows(d.cpu().numpy(), want, "play_moves records", moves)
    same_rows(planes.cpu().numpy(), host_planes(want), "play_moves planes", moves)
    seen = {k: int((want_st == k).sum()) for k in (0, -11, -12, -13, -14)}
    assert seen[-14] == 5 * n and seen[-11] >= 20 and seen[-13] >= 200 and seen[-12] > 10 * n and seen[0] > 5 * n, seen
    assert np.array_equal(want[want_st != 0], rows[want_st != 0])        # a refused move leaves the record alone
    # without planes, and rows that are left alone (move < 0) among rows that play
    d = dev(rows)
    assert np.array_equal(T.play_moves(d, dev(moves)).cpu().numpy(), want_st)
    same_rows(d.cpu().numpy(), want, "play_moves records, no planes", moves)
    some = moves.copy()
    some[::5] = -1 - (np.arange(len(some[::5])) % 3)
    want, want_st = host_play(rows, some)
    d = dev(rows)
    st = T.play_moves(d, dev(some), planes)
    assert np.array_equal(st.cpu().numpy(), want_st)
    same_rows(d.cpu().numpy(), want, "play_moves records, rows left alone", some)
    same_rows(planes.cpu().numpy(), host_planes(want), "play_moves planes, rows left alone", some)


@pytest.mark.parametrize("batch", [1, 2, 3, 4])
def test_play_moves_small_batches(corpus, recs, batch):
    """Three positions per workgroup: the captures, the kos and the suicides in every seat, alone and in a partial group."""
    cases = [("ring/b", 40), ("arms/b", 40), ("cap80_centre/b", 40), ("cap80_corner/w", 0), ("checker/b", 40),
             ("ko_centre/script1", 39), ("ko_edge/b", 3), ("ko_corner/b", 0), ("suicide3/b", 2), ("spiral/w", 48),
             ("eye_capture/b", 2), ("double/script1", 10), ("join4/b", 40), ("two_singles/b", 2)]
    base = recs[[A.index(n) for n, _ in cases]]
    moves = np.array([m for _, m in cases], np.int32)
    for shift in range(len(cases)):
        idx = np.roll(np.arange(len(cases)), shift)[:batch]
        want, want_st = host_play(base[idx], moves[idx])
        d = dev(base[idx])
        planes = torch.full((batch, 27, 9, 9), 99, dtype=torch.uint8, device=DEV)
        st = T.play_moves(d, dev(moves[idx]), planes)
        assert np.array_equal(st.cpu().numpy(), want_st), (shift, st, want_st)
        same_rows(d.cpu().numpy(), want, f"shift {shift}", moves[idx])
        same_rows(planes.cpu().numpy(), host_planes(want), f"planes, shift {shift}", moves[idx])
    st = host_play(base, moves)[1].tolist()
    assert st == [0, 0, 0, -13, 0, -11, 0, 0, -13, 0, 0, 0, 0, 0], st


def _script_rows(corpus):
    starts = np.stack([A.board_record(A.Case(s.name, s.board, None, None, s.turn)) for s in corpus.scripts])
    length = max(len(s.moves) for s in corpus.scripts)
    plan = np.full((len(starts), length), NONE, np.int32)
    for i, s in enumerate(corpus.scripts):
        plan[i, :len(s.moves)] = s.moves
    return starts, plan


def test_scripts_ply_by_ply(corpus):
    """The scripted sequences through bkt_play_moves and through bkt_playout_step, one launch per ply, the device playing on
    its own records: status, all 192 bytes and the planes after every ply.  bkt_play_moves leaves a row alone whose move is
    negative, so the passes of two scripts are played by the step alone (there the records are the corpus's own)."""
    starts, plan = _script_rows(corpus)
    for step in (False, True):
        host, d = starts.copy(), dev(starts)
        refused = accepted = 0
        for ply in range(plan.shape[1]):
            moves = plan[:, ply]
            planes = torch.full((len(host), 27, 9, 9), 99, dtype=torch.uint8, device=DEV)
            if step:
                playable = torch.full((len(host), 81), 99, dtype=torch.uint8, device=DEV)
                st = T.playout_step(d, dev(moves), None, planes, playable)
                want_st = np.array([A.play(host[i], m)[0] if m > NONE else 0 for i, m in enumerate(moves.tolist())])
                assert np.array_equal(st.cpu().numpy(), want_st), (ply, st, want_st)
                same_rows(playable.cpu().numpy(), RO.playable_host(host).astype(np.uint8), f"step playable, ply {ply}", moves)
            else:
                host, want_st = host_play(host, moves)
                st = T.play_moves(d, dev(moves), planes)
                assert np.array_equal(st.cpu().numpy(), want_st), (ply, st, want_st)
            same_rows(d.cpu().numpy(), host, f"{'step' if step else 'play_moves'} records, ply {ply}", moves)
            same_rows(planes.cpu().numpy(), host_planes(host), f"{'step' if step else 'play_moves'} planes, ply {ply}", moves)
            s = st.cpu().numpy()
            refused += int((s != 0).sum())
            accepted += int(((s == 0) & (moves > (NONE if step else -1))).sum())
        assert refused >= 12 and accepted >= 80, (step, refused, accepted)
        if step:                                                         # the step played the scripts as the corpus did
            for i, s in enumerate(corpus.scripts):
                last = [k for k, o in enumerate(corpus.origins) if o.kind == "script" and o.index == i][-1]
                assert np.array_equal(host[i, :81], corpus.recs[last, :81]), s.name


# ---- 3. bkt_playout_step -------------------------------------------------------------------------------------------------------
def check_step(recs, moves, over, want, **kw):
    """bkt_playout_step on the rows against want = test_gpu_rollout.host_step(recs, moves, over): records, status, over, and
    the planes and the playable set where they are asked for."""
    got = device_step(recs, moves, over, **kw)
    same_rows(got[0], want[0], "step records", moves)
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:8]
    if over is not None:
        assert np.array_equal(got[2], want[2]), np.nonzero(got[2] != want[2])[0][:8]
    assert (got[3] is None) == (not kw.get("want_planes", True)) and (got[4] is None) == (not kw.get("want_playable", True))
    if got[3] is not None:
        same_rows(got[3], want[3], "step planes", moves)
    if got[4] is not None:
        same_rows(got[4], want[4], "step playable", moves)


def test_playout_step_every_record_every_kind_of_row(recs):
    """play_moves' rows, and per record a pass, BKT_MOVE_NONE and a move below it; every seventh row with `over` set."""
    kinds = np.concatenate([MOVES, [go.PASS, NONE, NONE - 3]]).astype(np.int32)
    n = len(recs)
    rows = np.repeat(recs, len(kinds), 0)
    moves = np.tile(kinds, n)
    over = (np.arange(len(rows)) % 7 == 3).astype(np.uint8)
    assert len(rows) == 89 * n <= T.MAX_BATCH
    want, free = host_step(rows, moves, over), host_step(rows, moves, None)
    check_step(rows, moves, over, want)
    was_pass = L.record_last_move(rows) == go.PASS
    assert np.array_equal(want[2] > over, (moves == go.PASS) & (over == 0) & was_pass) and (want[2] > over).sum() >= 20
    assert np.array_equal(want[0][over != 0], rows[over != 0])           # an over row is untouched whatever its move
    seen = {k: int((want[1] == k).sum()) for k in (0, -11, -12, -13, -14)}
    assert seen[-14] > 4 * n and seen[-11] >= 15 and seen[-13] >= 150 and seen[-12] > 8 * n, seen
    empty = (want[4].sum(1) == 0).sum()
    assert empty > n, "rows without a playable point afterwards"
    check_step(rows, moves, None, free)                                  # over NULL: nothing ends, the over rows play
    check_step(rows, moves, over, want, want_planes=False)
    check_step(rows, moves, over, want, want_playable=False)
    check_step(rows, moves, None, free, want_planes=False, want_playable=False)


def test_playout_step_small_batches_and_the_playable_set(corpus, recs):
    """The playable set of every record as it stands (no move), in every seat and in batches of 1 to 4; then passes."""
    want = RO.playable_host(recs).astype(np.uint8)
    for idx, part in batches(recs):
        d = dev(part)
        playable = torch.full((len(part), 81), 99, dtype=torch.uint8, device=DEV)
        st = T.playout_step(d, torch.full((len(part),), NONE, dtype=torch.int32, device=DEV), None, None, playable)
        assert not st.any().item() and np.array_equal(d.cpu().numpy(), part)
        same_rows(playable.cpu().numpy(), want[idx], f"playable, {len(idx)} rows from {idx[0]}")
    for name, at in (("cap80_centre/b", [40]), ("cap80_corner/b", [0]), ("checker/b", [40]), ("cap80_centre/w", []),
                     ("cap80_corner/w", []), ("checker/w", [])):
        assert np.nonzero(want[A.index(name)])[0].tolist() == at, name
    for idx, part in A.small_batches(recs, rows=(1, 3, 4)):
        moves = np.full(len(part), go.PASS, np.int32)
        over = np.zeros(len(part), np.uint8)
        check_step(part, moves, over, host_step(part, moves, over))


# ---- 4. the score --------------------------------------------------------------------------------------------------------------
def test_area_score_and_owner(recs):
    want_owner = RO.owner_host(recs)
    want = L.area_score_host(recs, 5.5).astype(np.float32)
    flood = (want_owner > 0).sum(1).astype(np.float32) - ((want_owner < 0).sum(1).astype(np.float32) + np.float32(5.5))
    assert np.array_equal(want, flood)                                   # the C function and the Python flood
    for idx, part in batches(recs):
        d = dev(part)
        score, owner = T.area_score(d, 5.5, owner=True)
        assert np.array_equal(score.cpu().numpy().view(np.int32), want[idx].view(np.int32)), idx[:4]
        same_rows(owner.cpu().numpy(), want_owner[idx], f"owner, {len(idx)} rows from {idx[0]}")
        assert np.array_equal(d.cpu().numpy(), part)
    plain = T.area_score(dev(recs), 5.5)
    assert np.array_equal(plain.cpu().numpy().view(np.int32), want.view(np.int32))
    corridor = sorted(A.flood(A.SPIRAL, 9)[1])                           # 31 rounds deep: black's alone, or nobody's
    assert (want_owner[A.index("spiral/b")] == 1).all() and (want_owner[A.index("spiral_swapped/b")] == -1).all()
    assert (want_owner[A.index("spiral_two/w")][corridor] == 0).all()


@pytest.mark.parametrize("records,playouts", [(1, 1), (3, 7), (5, 4)])
def test_owner_counts(recs, records, playouts):
    n, rows = len(recs), records * playouts
    ran = 0
    for lo in range(0, n, rows):
        part = np.ascontiguousarray(recs[np.arange(lo, lo + rows) % n])
        got = T.owner_counts(dev(part), records, playouts, 5.5)
        want = RO.owner_counts_host(part, records, playouts, 5.5)
        for g, w, what in zip(got, want, ("black", "white", "agree", "hist", "black_wins")):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, lo)
        ran += rows
    assert ran >= n


# ---- 5. the codes and the weights ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """test_gpu_tactics.py's seeded tables over the whole uint16 range."""
    rng = np.random.default_rng(17)
    w = rng.integers(0, 65536, PT.ENTRIES).astype(np.uint16)
    w[rng.integers(0, PT.ENTRIES, 4096)] = 0
    w[rng.integers(0, PT.ENTRIES, 4096)] = 65535
    w[0], w[1 << 16] = 0, 65535
    rng = np.random.default_rng(23)
    t = rng.integers(0, 65536, TC.ENTRIES).astype(np.uint16)
    t[8], t[4], t[9], t[20] = 65535, 0, 65535, 0
    return PT.PatternTable(w), TC.TacticTable(t)


def test_pattern_and_tactical_codes(recs):
    want_p, want_t = PT.codes_host(recs), TC.codes_host(recs)
    assert ((want_t & 3) > 0).any() and ((want_t >> 4) & 1).any() and ((want_t >> 5) & 1).any()
    for idx, part in batches(recs):
        d = dev(part)
        same_rows(T.pattern_codes(d).cpu().numpy(), want_p[idx].astype(np.int32), f"pattern codes from {idx[0]}")
        same_rows(T.tactical_codes(d).cpu().numpy(), want_t[idx].astype(np.int32), f"tactical codes from {idx[0]}")
        assert np.array_equal(d.cpu().numpy(), part)


@pytest.mark.parametrize("with_patterns,with_tactics", [(False, False), (True, False), (False, True), (True, True)])
def test_move_weights(recs, tables, with_patterns, with_tactics):
    p, t = tables[0] if with_patterns else None, tables[1] if with_tactics else None
    want = RO.move_weights_host(recs, p, t)
    assert np.array_equal(want != 0, RO.playable_host(recs))             # a playable point weighs at least 1
    args = (None if p is None else p.device(DEV), None if t is None else t.device(DEV))
    for idx, part in batches(recs):
        d = dev(part)
        same_rows(T.move_weights(d, *args).cpu().numpy(), want[idx], f"move weights from {idx[0]}")
        assert np.array_equal(d.cpu().numpy(), part)


# ---- 6. the ply loops ------------------------------------------------------------------------------------------------------------
def _reply_tables():
    rng = np.random.default_rng(41)
    single = rng.integers(0, 81, (2, 81)).astype(np.uint8)
    single[rng.random((2, 81)) < 0.3] = 255                             # BKT_REPLY_NONE
    pairs = rng.integers(0, 81, (2, 82, 81)).astype(np.uint8)
    pairs[rng.random((2, 82, 81)) < 0.5] = 255
    return single, pairs


def _values():
    v = np.random.default_rng(30).integers(1, 65536, (2, 81)).astype(np.uint16)
    v[0, ::7], v[1, 3::5], v[:, 40] = 1, 65535, (65535, 1)
    return MV.MoveValueTable(np.zeros((2, 81, 2), np.int64), v, MV.lut_of(1.0), 1, 0)


LOOPS = ("random", "pattern", "tactical", "reply", "reply2", "move_value")


def _loop_tables(kind, tables):
    """The keyword arguments of rollout.random_playouts for the kernel `kind`, tables that are not neutral; a fresh copy
    per call of the tables that the call updates afterwards."""
    single, pairs = _reply_tables()
    return {"random": {}, "pattern": dict(patterns=tables[0]), "tactical": dict(patterns=tables[0], tactics=tables[1]),
            "reply": dict(patterns=tables[0], tactics=tables[1], replies=RO.ReplyTable(single)),
            "reply2": dict(patterns=tables[0], tactics=tables[1], replies=RO.ReplyTable2(pairs)),
            "move_value": dict(patterns=tables[0], tactics=tables[1], move_values=_values())}[kind]


@pytest.mark.parametrize("kind", LOOPS)
def test_ply_loops_from_corpus_starts(corpus, recs, tables, kind):
    """bkt_random_playouts, bkt_pattern_playouts, bkt_tactical_playouts, bkt_reply_playouts, bkt_reply2_playouts and
    bkt_move_value_playouts: three playouts of 24 plies from every record against the host mirror."""
    starts = np.repeat(recs, PLAYOUTS, 0)
    host_kw, dev_kw = _loop_tables(kind, tables), _loop_tables(kind, tables)
    host = RO.random_playouts(starts, SEED, max_plies=CAP, rules="host", **host_kw)
    got = RO.random_playouts(starts, SEED, max_plies=CAP, **dev_kw)
    _assert_same(got, host, kind)
    assert len(host.plies) == PLAYOUTS * len(recs) and host.moves.shape[1] == CAP
    for name, at in (("cap80_centre/b", 40), ("cap80_corner/b", 0), ("checker/b", 40), ("cap80_centre_white/w", 40),
                     ("cap80_centre/w", go.PASS), ("cap80_corner/w", go.PASS), ("checker/w", go.PASS)):
        i = PLAYOUTS * A.index(name)
        assert host.moves[i:i + PLAYOUTS, 0].tolist() == [at] * PLAYOUTS, (name, host.moves[i:i + PLAYOUTS, 0])
        assert got.moves[i:i + PLAYOUTS, 0].tolist() == [at] * PLAYOUTS, name
    if kind in ("reply", "reply2"):                                      # the tables both calls then learned from their games
        assert host.reply_plies > 100, host.reply_plies
        assert np.array_equal(dev_kw["replies"].array, host_kw["replies"].array)
    if kind == "move_value":
        assert np.array_equal(dev_kw["move_values"].counts, host_kw["move_values"].counts)
        assert np.array_equal(dev_kw["move_values"].values, host_kw["move_values"].values)
    # the same games in batches of 1 to 4 rows (a row's game depends on its record, its counters and the tables alone)
    ctr = RO.default_counters(len(starts), RO.record_turns(starts))
    hard = [PLAYOUTS * A.index(n) for n in ("spiral/w", "ring/b", "arms/b", "cap80_centre/b", "checker/w", "ko_corner/script1")]
    for rows in (1, 2, 3, 4):
        for lo in hard:
            sub = RO.random_playouts(starts[lo:lo + rows], SEED, counters=ctr[lo:lo + rows], max_plies=CAP,
                                     **_loop_tables(kind, tables))
            assert np.array_equal(sub.records.cpu().numpy(), host.records[lo:lo + rows]), (kind, rows, lo)
            assert np.array_equal(sub.moves, host.moves[lo:lo + rows, :sub.moves.shape[1]]), (kind, rows, lo)
            assert np.array_equal(sub.plies, host.plies[lo:lo + rows])

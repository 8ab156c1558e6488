"""CPU: the move weights of a position and the pattern term of the search prior, as far as they need no GPU --
the host mirror of bkt_move_weights against hand-written cases and against the first plies of the host playouts,
amaf_prior(weights=, mu=) and pattern_prior, PlayoutEvaluator(pattern_prior=) and the tree on the host rules, the keywords
and the command lines, the declaration, the binding and the build, and the kernel's resources when compiled for gfx950."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, selfplay
from bokego_amd import lockstep as L
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN, REPO
from test_amaf_cpu import BOARD, records, seeded_tables, three_records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
SEED = 5
NEUTRAL_P = PT.PatternTable.constant(256)
NEUTRAL_T = TC.TacticTable.neutral()


def golden_records():
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


def played_records(games=2):
    """Golden playouts replayed with bk_pos_play alone: the liberty cache is valid and a refresh is pending on it."""
    from bokego_amd import reinforce as R
    play, out = R._play_fn(), []
    for moves in json.load(open(os.path.join(GOLDEN, "playouts.json")))["moves"][:games]:
        rec = R.initial_positions(1)
        for mv in moves:
            assert play(rec.ctypes.data, int(mv)) == 0
            out.append(rec[0].copy())
    return np.stack(out)


def ko_record():
    """White to move after black has taken the ko at 11: the ko point is 10."""
    g = go.Game(board="".join([".XO......", "XO.O.....", ".XO......"] + ["........."] * 6))
    g.play_move(11)
    rec = records([g])
    assert L.record_last_move(rec)[0] == 11 and rec[0, 10] == 0 and int(rec[0, 164:166].view(np.int16)[0]) == 10
    return rec


def eyes_only_record():
    """BOARD after black's capture at 38: white to move, and every empty point is an eye or a suicide."""
    g = go.Game(BOARD)
    g.play_move(38)
    rec = records([g])
    assert not RO.playable_host(rec).any() and (rec[0, :81] == 0).sum() == 4
    return rec


def first_moves(recs, pat, tac, n=7, rules="host", **kw):
    """The first moves of n one-ply playouts per record and the ply-0 Philox words they were drawn with."""
    rows = np.repeat(recs, n, 0)
    fin = RO.random_playouts(rows, SEED, max_plies=1, rules=rules, patterns=pat, tactics=tac, **kw)
    ctr = RO.default_counters(len(rows), RO.record_turns(rows)).view(np.uint32)
    x0 = L.philox4x32_10(ctr, L.seed_key(L.seed_u64(SEED)))[:, 0]
    return fin.moves[:, 0].reshape(len(recs), n), x0.reshape(len(recs), n)


def check_first_moves(weights, moves, x0):
    """patterns.weighted_pick on the ply-0 word, over the non-zero weights in ascending point order, gives every playout's
    first move; a row whose weights are all zero passes."""
    for r in range(len(weights)):
        pts = np.nonzero(weights[r])[0]
        for j in range(moves.shape[1]):
            want = go.PASS if len(pts) == 0 else int(pts[PT.weighted_pick(x0[r, j], weights[r][pts])])
            assert moves[r, j] == want, (r, j, moves[r, j], want)


# ---- 1. hand-written cases ------------------------------------------------------------------------------------------------------
def test_hand_written_weights():
    g = go.Game()
    g.play_move(40)
    one = records([g])                                                # a single black stone, white to move
    w = np.full(PT.ENTRIES, 256, np.uint16)
    w[PT.NEAR | 2 << 2] = 1000                                        # point 31: the opponent's stone in slot (+1, 0), near
    assert PT.codes_host(one)[0, 31] == (PT.NEAR | 8) and (PT.codes_host(one)[0] == (PT.NEAR | 8)).sum() == 1
    got = RO.move_weights_host(one, w)
    assert got.dtype == np.int32 and got.shape == (1, 81)
    assert got[0, 31] == 1000 and got[0, 40] == 0 and (np.delete(got[0], [31, 40]) == 256).all()
    t = np.full(TC.ENTRIES, 256, np.uint16)
    code = int(TC.codes_host(one)[0, 31])
    t[code] = 512
    both = RO.move_weights_host(one, w, t)
    assert both[0, 31] == 2000 and both[0, 40] == 0
    assert np.array_equal(both[0] == 512, (TC.codes_host(one)[0] == code) & (np.arange(81) != 31) & (np.arange(81) != 40))
    w[PT.NEAR | 8], t[code] = 0, 1                                    # P = max(0, 1) = 1, T = 1: w = max(1, 1 >> 8) = 1
    assert RO.move_weights_host(one, w, t)[0, 31] == 1
    # a record whose last move is a pass: near = 0 everywhere
    passed = three_records()[2:3]
    assert L.record_last_move(passed)[0] == go.PASS
    w = np.full(PT.ENTRIES, 256, np.uint16)
    w[PT.NEAR:] = 999
    got = RO.move_weights_host(passed, w)
    assert got[0, 40] == 0 and (np.delete(got[0], 40) == 256).all()
    # a ko point has weight 0, whatever the tables say
    ko = ko_record()
    got = RO.move_weights_host(ko, *seeded_tables())
    assert got[0, 10] == 0 and not RO.legal_host(ko)[0, 10]
    assert (got[0] > 0).sum() == (ko[0, :81] == 0).sum() - 2         # the ko point, and white's suicide at 0
    # a legal own eye has weight 0
    z = np.load(os.path.join(GOLDEN, "possible_eye.npz"))
    lib, found = go.golib(), 0
    for b in z["boards"][::40]:
        for turn in (0, 1):
            rec = records([go.Game(board="".join(".XO"[c] for c in b), turn=turn)])
            legal = RO.legal_host(rec)[0]
            eyes = [s for s in np.nonzero(legal)[0] if lib.bk_pos_possible_eye(L.pos_ptr(rec[0]), int(s)) == 1 + turn]
            got = RO.move_weights_host(rec, None, None)[0]
            assert all(got[s] == 0 for s in eyes) and np.array_equal(got > 0, legal & ~np.isin(np.arange(81), eyes))
            found += len(eyes)
    assert found > 10
    assert not RO.move_weights_host(eyes_only_record(), *seeded_tables()).any()


# ---- 2. the mirror against the first plies of the host playouts --------------------------------------------------------------------
def test_mirror_gives_the_first_moves_of_the_host_playouts():
    gold = golden_records()
    recs = np.ascontiguousarray(np.concatenate([gold[30::len(gold) // 8][:8], played_records(1)[20:22], ko_record(),
                                                eyes_only_record(), three_records()[2:3]]))
    pat, tac = seeded_tables()
    for p, t in ((pat, tac), (None, tac), (pat, NEUTRAL_T)):
        w = RO.move_weights_host(recs, p, t)
        assert np.array_equal(w > 0, RO.playable_host(recs)) and w.max() < 1 << 24
        check_first_moves(w, *first_moves(recs, p, t))
    assert not RO.move_weights_host(recs, pat, tac)[-2].any()          # the eyes-only record: every playout passes
    # both tables neutral, or none: 256 times the playable set
    want = 256 * RO.playable_host(recs).astype(np.int32)
    assert np.array_equal(RO.move_weights_host(recs, NEUTRAL_P, NEUTRAL_T), want)
    assert np.array_equal(RO.move_weights_host(recs), want)
    assert np.array_equal(RO.move_weights(recs, rules="host"), want)
    before = recs.copy()
    RO.move_weights_host(recs, pat, tac)
    assert np.array_equal(recs, before)
    with pytest.raises(ValueError):
        RO.move_weights_host(recs[:, :100])
    with pytest.raises(ValueError):
        RO.move_weights(recs, rules="gpu")


# ---- 3. amaf_prior and pattern_prior --------------------------------------------------------------------------------------------
def _amaf(played, won, wins, n):
    return RO.Amaf(None, np.asarray(wins, np.int32), np.asarray(played, np.int32), np.asarray(won, np.int32), n)


def test_amaf_prior_with_weights():
    recs = np.ascontiguousarray(np.concatenate([three_records(), ko_record()]))
    a = RO.playout_amaf(recs, 6, SEED, rules="host")
    w = RO.move_weights_host(recs, *seeded_tables())
    crit = np.random.default_rng(3).uniform(-0.2, 0.2, (4, 81))
    # mu = 0 and weights=None: today's floats, bit for bit, with and without criticality
    for kw in ({}, dict(criticality=crit, gamma=0.7), dict(k=1.0, temperature=0.5)):
        old = RO.amaf_prior(recs, a, **kw)
        for more in (dict(weights=w, mu=0.0), dict(weights=None, mu=2.0), dict(weights=None), dict(mu=0.0)):
            assert np.array_equal(old.view(np.int32), RO.amaf_prior(recs, a, **kw, **more).view(np.int32)), (kw, more)
    # the documented logits
    legal = RO.legal_host(recs)
    q = (a.won + 4.0 * (a.wins / 6.0)[:, None]) / (a.played + 4.0) + 0.7 * crit
    z = q / 0.1 + 1.5 * np.log(np.maximum(w.astype(np.float64), 1.0))
    z = np.where(legal, z, -np.inf)
    p = np.where(legal, np.exp(z - z.max(1, keepdims=True)), 0.0)
    want = (p / p.sum(1, keepdims=True)).astype(np.float32)
    got = RO.amaf_prior(recs, a, criticality=crit, gamma=0.7, weights=w, mu=1.5)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got > 0, legal) and np.allclose(got.sum(1), 1.0, atol=1e-6)
    # mu flips the top prior: AMAF prefers 12 (8 of 8 won against 6 of 8), the weights prefer 11 by a factor of 2^12
    played, won = np.zeros((1, 81)), np.zeros((1, 81))
    played[0, [11, 12]], won[0, [11, 12]] = 8, [6, 8]
    one = _amaf(played, won, [8], 16)
    ww = np.full((1, 81), 16, np.int32)
    ww[0, 11] = 1 << 16
    assert RO.amaf_prior(recs[1:2], one, weights=ww, mu=0.0)[0].argmax() == 12
    assert RO.amaf_prior(recs[1:2], one, weights=ww, mu=0.1)[0].argmax() == 12     # (2 / 12) / 0.1 > 0.1 * 12 ln 2
    assert RO.amaf_prior(recs[1:2], one, weights=ww, mu=1.0)[0].argmax() == 11
    # a legal point off the playable set (an own eye) enters with weight 1, not 0
    eye = records([go.Game(BOARD)])
    assert RO.legal_host(eye)[0, 0] and not RO.playable_host(eye)[0, 0]
    p = RO.amaf_prior(eye, _amaf(np.zeros((1, 81)), np.zeros((1, 81)), [3], 6), weights=np.where(np.arange(81) == 38, 4, 0)[None],
                      mu=1.0)[0]
    assert p[0] > 0 and np.isclose(p[38] / p[0], 4.0) and np.isfinite(p).all()
    # pattern_prior: the table's own prediction
    pp = RO.pattern_prior(recs, w)
    assert pp.dtype == np.float32 and pp.shape == (4, 81) and np.allclose(pp.sum(1), 1.0, atol=1e-6)
    assert np.array_equal(pp > 0, legal) and pp[3, 10] == 0
    row = np.maximum(w[1].astype(np.float64), 1.0) * legal[1]
    assert np.allclose(pp[1], row / row.sum(), rtol=1e-6)
    assert np.allclose(RO.pattern_prior(recs, w, mu=0.0)[1], legal[1] / legal[1].sum())
    full = np.frombuffer(bytes(go.Game(BOARD)._pos), np.uint8).copy()
    full[:81][full[:81] == 0] = 1                                     # a board without an empty point
    assert np.array_equal(RO.pattern_prior(full[None], np.zeros((1, 81), np.int32)), np.full((1, 81), 1 / 81, np.float32))
    assert np.array_equal(RO.amaf_prior(full[None], _amaf(np.ones((1, 81)), np.zeros((1, 81)), [1], 4),
                                        weights=np.ones((1, 81), np.int32), mu=1.0), np.full((1, 81), 1 / 81, np.float32))
    # what is refused
    for kw in (dict(mu=-0.5), dict(mu=float("nan")), dict(mu=float("inf")), dict(weights=w[:2], mu=1.0),
               dict(weights=w.reshape(-1), mu=1.0), dict(weights=w, mu=-1.0)):
        with pytest.raises(ValueError):
            RO.amaf_prior(recs, a, **kw)
    for args in ((recs, w, -1.0), (recs, w, float("nan")), (recs, w[:3], 1.0)):
        with pytest.raises(ValueError):
            RO.pattern_prior(*args)


# ---- 4. the evaluator, the search and the flags ---------------------------------------------------------------------------------
def test_playout_evaluator_with_a_pattern_prior():
    recs = three_records()
    pat, tac = seeded_tables()
    same = lambda x: x                                                # noqa: E731
    carried = lambda h: {f for f, x in vars(h.run).items() if x is not None}   # noqa: E731  (what a request's run holds)
    for rave in (False, True):
        for gamma in (0.0, 0.5):
            base = dict(seed=4, rules="host", prior=1.0, rave=rave, criticality=gamma)
            # mu = 0: the handle and the results are what they are without the keywords
            old = RO.PlayoutEvaluator(None, 2, **base)
            off = RO.PlayoutEvaluator(None, 2, pattern_prior=0.0, prior_patterns=pat, prior_tactics=tac, **base)
            h_old, h_off = old.submit(recs, 2), off.submit(recs, 2)
            assert h_old.weights is None and h_off.weights is None and carried(h_old) == carried(h_off)
            r_old, r_off = old.finish(h_old), off.finish(h_off)
            assert len(r_old) == len(r_off) == 2 + rave
            assert np.array_equal(r_old[0], r_off[0]) and np.array_equal(r_old[1], r_off[1])
            # mu > 0: amaf_prior with the mirror's weights of the first n_policy rows
            ev = RO.PlayoutEvaluator(None, 2, pattern_prior=1.5, prior_patterns=pat, prior_tactics=tac, **base)
            h = ev.submit(recs, 2)
            assert h.weights is not None and carried(h) == carried(h_old)
            assert np.array_equal(h.weights, RO.move_weights_host(recs[:2], pat, tac))
            out = ev.finish(h, normalise=same)
            a = RO.playout_amaf(recs[:2], 2, 4, rules="host")
            crit = RO.playout_ownership(recs[:2], 2, 4, rules="host").criticality() if gamma else None
            want = RO.amaf_prior(recs[:2], a, criticality=crit, gamma=gamma, weights=RO.move_weights_host(recs[:2], pat, tac),
                                 mu=1.5)
            assert np.array_equal(out[0].view(np.int32), want.view(np.int32)) and not np.array_equal(out[0], r_old[0])
            assert np.array_equal(out[1], r_old[1])                   # the values of all rows
            if rave:
                assert out[2][0] == r_old[2][0] and all(np.array_equal(x, y) for x, y in zip(out[2][1:], r_old[2][1:]))
            p, v = ev(recs, 0)[:2]                                    # no policy rows: nothing to weigh
            assert p.shape == (0, 81) and np.array_equal(v, r_old[1])
    # the tables of the prior default to the playouts' own
    ev = RO.PlayoutEvaluator(None, 2, seed=4, rules="host", prior=1.0, pattern_prior=1.0, patterns=pat, tactics=tac)
    assert ev.prior_patterns is ev.patterns and ev.prior_tactics is ev.tactics
    own = ev.finish(ev.submit(recs, 2), normalise=same)[0]
    a = RO.playout_amaf(recs[:2], 2, 4, rules="host", patterns=pat, tactics=tac)
    assert np.array_equal(own, RO.amaf_prior(recs[:2], a, weights=RO.move_weights_host(recs[:2], pat, tac), mu=1.0))
    ev = RO.PlayoutEvaluator(None, 2, rules="host", prior=1.0, pattern_prior=1.0, patterns=pat, prior_tactics=tac.array)
    assert ev.prior_patterns is ev.patterns and ev.tactics is None and np.array_equal(ev.prior_tactics.array, tac.array)
    # a policy engine's share is mixed as before
    from test_amaf_cpu import _FakeEngine
    ev = RO.PlayoutEvaluator(_FakeEngine(), 2, seed=4, rules="host", prior=0.5, pattern_prior=1.0, prior_patterns=pat)
    ph = ev.finish(ev.submit(recs, 2), normalise=same)[0]
    pi = _FakeEngine().submit_positions(recs[:2], False, True, False, 2)
    mine = RO.amaf_prior(recs[:2], RO.playout_amaf(recs[:2], 2, 4, rules="host"),
                         weights=RO.move_weights_host(recs[:2], pat), mu=1.0)
    assert np.array_equal(ph, (0.5 * pi.astype(np.float64) + 0.5 * mine.astype(np.float64)).astype(np.float32))
    # what is refused
    with pytest.raises(ValueError, match="prior > 0"):
        RO.PlayoutEvaluator(_FakeEngine(), 2, rules="host", pattern_prior=1.0, prior_patterns=pat)
    with pytest.raises(ValueError, match="table"):
        RO.PlayoutEvaluator(None, 2, rules="host", prior=1.0, pattern_prior=1.0)
    for mu in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            RO.PlayoutEvaluator(None, 2, rules="host", prior=1.0, pattern_prior=mu, prior_patterns=pat)


def test_native_mcts_with_a_pattern_prior_is_deterministic():
    r = max(json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"], key=lambda r: sum(c != "." for c in r["board"]))
    pat, tac = seeded_tables()
    seen = []
    for seed in (SEED, SEED, SEED + 1):
        t = NativeMCTS(Position(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"]), None, None,
                       playout_value=2, playout_prior=1, playout_pattern_prior=1, playout_rave=4, prior_patterns=pat,
                       prior_tactics=tac, expand_thresh=3, playout_seed=seed, playout_rules="host")
        ev = t.evaluator
        assert ev.pattern_prior == 1.0 and ev.prior_patterns is pat and ev.prior_tactics is tac and ev.patterns is None
        t.rollout(40)
        seen.append(({mv: n for mv, (n, _) in t.child_stats().items()}, t.choose().last_move))
        t.close()
    assert seen[0] == seen[1] and sum(seen[0][0].values()) == 40 and seen[0][1] in seen[0][0]
    t = NativeMCTS(Position(board=BOARD), None, None, playout_value=2, playout_prior=1.0, playout_rules="host",
                   playout_patterns=pat, playout_pattern_prior=0.5, expand_thresh=1)
    assert t.evaluator.prior_patterns is t.evaluator.patterns and t.evaluator.pattern_prior == 0.5
    t.rollout(6)
    assert t.choose().last_move == 38
    t.close()
    t = NativeMCTS(Position(board=BOARD), None, None, playout_value=2, playout_prior=1.0, playout_rules="host")
    assert t.evaluator.pattern_prior == 0.0 and t.playout_pattern_prior == 0.0
    t.close()
    for kw in (dict(playout_pattern_prior=1.0, prior_patterns=pat), dict(prior_tactics=tac)):
        with pytest.raises(TypeError, match="playout_prior"):
            NativeMCTS(Position(), None, None, playout_value=2, playout_rules="host", evaluator=None, **kw)
    with pytest.raises(ValueError):
        NativeMCTS(Position(), None, None, playout_value=2, playout_prior=1.0, playout_pattern_prior=-1.0,
                   prior_patterns=pat, playout_rules="host")
    with pytest.raises(ValueError, match="table"):
        NativeMCTS(Position(), None, None, playout_value=2, playout_prior=1.0, playout_pattern_prior=1.0, playout_rules="host")


def test_command_lines(capsys):
    base = ["--playout-value", "64", "--playout-prior", "1"]
    for mod in (gtp, match, selfplay):
        a = mod.parse_args([])
        assert (a.playout_pattern_prior, a.prior_patterns, a.prior_tactics) == (0.0, None, None)
        a = mod.parse_args(base + ["--playout-pattern-prior", "0.5", "--prior-patterns", "p.npy", "--prior-tactics", "t.npy"])
        assert (a.playout_pattern_prior, a.prior_patterns, a.prior_tactics) == (0.5, "p.npy", "t.npy")
        a = mod.parse_args(base + ["--playout-pattern-prior", "2", "--playout-tactics", "t.npy"])
        assert (a.playout_pattern_prior, a.prior_patterns, a.playout_tactics) == (2.0, None, "t.npy")
        for bad in (["--playout-value", "64", "--playout-pattern-prior", "1", "--prior-patterns", "p.npy"],   # no --playout-prior
                    ["--playout-pattern-prior", "1", "--prior-patterns", "p.npy"],
                    base + ["--playout-pattern-prior", "1"],                                                 # no table at all
                    base + ["--playout-pattern-prior", "-1", "--prior-patterns", "p.npy"],
                    base + ["--playout-pattern-prior", "nan", "--prior-patterns", "p.npy"],
                    base + ["--playout-pattern-prior", "inf", "--prior-patterns", "p.npy"],
                    base + ["--playout-pattern-prior", "x", "--prior-patterns", "p.npy"],
                    base + ["--prior-patterns", "p.npy"], base + ["--prior-tactics", "t.npy"]):
            with pytest.raises(SystemExit):
                mod.parse_args(bad)
    a = RO._parse(["--sgf", "g.sgf", "--random", "--weights", "--patterns", "p.npy"])
    assert a.weights is True and a.patterns == "p.npy" and RO._parse(["--sgf", "g.sgf", "--random"]).weights is False
    for bad in (["--sgf", "g.sgf", "--weights"], ["--sgf", "g.sgf", "--random", "--weights", "--amaf"],
                ["--sgf", "g.sgf", "--random", "--weights", "--ownership"], ["--sgf", "g.sgf", "--weights", "-p", "w.bkw"]):
        with pytest.raises(SystemExit):
            RO._parse(bad)
    capsys.readouterr()


# ---- 5. header, library, Makefile, kernel -----------------------------------------------------------------------------------------
def test_header_binding_and_build_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_move_weights\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*int\s+batch\s*,"
                     r"\s*const\s+uint16_t\s*\*\s*table\s*,\s*const\s+uint16_t\s*\*\s*tactics\s*,"
                     r"\s*uint32_t\s*\*\s*weights\s*,\s*void\s*\*\s*stream\s*\)", code)
    comment = re.sub(r"\s*\n \*\s*", " ", src[:src.index("int bkt_move_weights")].rsplit("/*", 1)[1])
    for phrase in ("weights[b*81 + s]", "first ply", "bkt_tactical_playouts' draw", "fresh = 0", "bk_pos_possible_eye",
                   "bkt_playout_step leaves behind for an untouched record", "P = max(table[index], 1)",
                   "exactly bkt_pattern_codes' index", "P = 256 when table is NULL", "T = tactics[code]",
                   "exactly bkt_tactical_codes' code", "T = 256 when tactics is NULL", "w_s = max(1, (P * T) >> 8)",
                   "0 off it", "both may be NULL", "256 on the playable set", "read only", "Integers only",
                   "1 <= batch <= BKT_MAX_BATCH", "BKT_ERR_ARG", "nothing written"):
        assert phrase in comment, phrase
    P, I = ctypes.c_void_p, ctypes.c_int
    assert T.SYMBOLS["bkt_move_weights"] == (I, [P, I, P, P, P, P]) and callable(T.move_weights)
    for name in ("move_weights", "move_weights_host", "pattern_prior", "amaf_prior"):
        assert name in RO.__all__
    assert all(hasattr(RO, name) for name in RO.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_move_weights
    make = open(os.path.join(CSRC, "Makefile")).read()
    (line,) = [l for l in make.splitlines() if l.startswith("\t") and "-o $@" in l and "bk_playout_pat.hip" in l]
    words = line.split()
    assert "bk_playout_prior.hip" in words
    assert words.index("bk_playout_owner.hip") < words.index("bk_playout_prior.hip") < words.index("-shared")
    assert "-shared bk_train.hip bk_train_bf16.hip bk_playout_pat.hip -o" in line
    (rule,) = [l for l in make.splitlines() if l.startswith("$(TRAIN_OUT):")]
    assert "bk_playout_prior.hip" in rule.split()
    for name in ("bk_playout.hip", "bk_playout_mc.hip", "bk_playout_pat.hip", "bk_playout_tac.hip", "bk_playout_amaf.hip",
                 "bk_playout_rave.hip", "bk_playout_owner.hip"):
        assert "bk_playout_prior" not in open(os.path.join(CSRC, name)).read()
    own = open(os.path.join(CSRC, "bk_playout_prior.hip")).read()
    assert '#include "bk_encode_dev.h"' in own and not re.search(r'#include\s+"bk_playout', own)
    assert "repeated here on purpose" in own and "atomic" not in own.replace("no atomics", "")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_builds_alone_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_prior.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    assert len(blocks) == 1 and "move_weights_kernel" in blocks[0].split()[0], [b.split()[0] for b in blocks]
    field = lambda pat: int(re.search(pat + r": (\d+)", blocks[0]).group(1))  # noqa: E731
    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field(r"SGPRs Spill") == 0 and field(r"VGPRs Spill") == 0, blocks[0]
    # the encoder's LDS -- two ballot buffers of 8 words and a uint4 per point of three records -- and two more ballot
    # buffers for the neighbour bits
    assert field(r"LDS Size \[bytes/block\]") == 2 * 8 * 4 + 3 * 81 * 16 + 2 * 8 * 4 == 4016, blocks[0]
    assert field(r" VGPRs") <= 64 and field(r"Occupancy \[waves/SIMD\]") == 8, blocks[0]

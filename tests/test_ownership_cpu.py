"""CPU: ownership and criticality from the playouts, as far as they need no GPU -- the declaration and the
binding of bkt_owner_counts, its host mirror against counts written out by hand and against owner_host reduced in plain
numpy, playout_ownership on the host rules, the criticality term of amaf_prior, PlayoutEvaluator(criticality=), the
keywords and the command lines, the net-free GTP engine's score by playouts, and the kernel's resources when compiled for
gfx950."""
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
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import GOLDEN, REPO
from test_amaf_cpu import BOARD, records, three_records

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
COUNTS = ("black", "white", "agree", "hist", "black_wins")

# One record x 3 boards, komi 5.5:
#   A  no stone: the one empty region touches nobody, nobody owns anything; d = 0, white wins by komi.
#   B  one black stone at 40: the stone and the black-only region, all 81 points black's; d = 81, black wins.
#   C  black at 0, white at 80: the one empty region touches both and is neutral; d = 1 - 1 = 0, white wins.
HAND_BOARDS = ("." * 81, "." * 40 + "X" + "." * 40, "X" + "." * 79 + "O")
HAND_BLACK = np.ones((1, 81), np.int32)            # B everywhere ...
HAND_BLACK[0, 0] = 2                               # ... and C's stone
HAND_WHITE = np.zeros((1, 81), np.int32)
HAND_WHITE[0, 80] = 1                              # C's stone
HAND_AGREE = np.ones((1, 81), np.int32)            # B: black's points, black won.  C: black's stone lost ...
HAND_AGREE[0, 80] = 2                              # ... and white's stone is the winner's
HAND_HIST = np.zeros((1, 163), np.int32)
HAND_HIST[0, 81], HAND_HIST[0, 162] = 2, 1
HAND_WINS = np.array([1], np.int32)
HAND = (HAND_BLACK, HAND_WHITE, HAND_AGREE, HAND_HIST, HAND_WINS)


def hand_records():
    return records([go.Game(b) for b in HAND_BOARDS])


def reduced(own, score_positive, records_, playouts):
    """bkt_owner_counts' definition on an owner array [G,81] and the rows black won, in plain numpy loops."""
    own = np.asarray(own, np.int64)
    out = [np.zeros((records_, 81), np.int32) for _ in range(3)] + [np.zeros((records_, 163), np.int32),
                                                                   np.zeros(records_, np.int32)]
    for g in range(records_ * playouts):
        r, bw = g // playouts, bool(score_positive[g])
        out[0][r] += own[g] == 1
        out[1][r] += own[g] == -1
        out[2][r] += ((own[g] == 1) & bw) | ((own[g] == -1) & (not bw))
        out[3][r, int((own[g] == 1).sum() - (own[g] == -1).sum()) + 81] += 1
        out[4][r] += bw
    return tuple(out)


def same_counts(a, b):
    for x, y, name in zip(a, b, COUNTS):
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape, name
        assert np.array_equal(x, y), (name, np.argwhere(x != y)[:8])


def golden_records():
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"]
    return np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"],
                                                 turn=r["turn"])._pos), np.uint8) for r in pos])


# ---- 1. the mirror ---------------------------------------------------------------------------------------------------------------
def test_host_counts_equal_the_hand_written_ones():
    got = RO.owner_counts_host(hand_records(), 1, 3, 5.5)
    same_counts(got, HAND)
    o = RO.Ownership(None, None, *got, 3)
    crit = o.criticality()
    assert crit.dtype == np.float64 and crit.shape == (1, 81)
    assert crit[0, 80] == 2 / 3 - (1 / 3 * (1 / 3) + 1 / 3 * (1 - 1 / 3)) and abs(crit[0, 80] - 1 / 3) < 1e-15
    assert np.array_equal(o.mean_owner[0, [0, 1, 80]], [2 / 3, 1 / 3, 0.0]) and o.mean_margin[0] == 27.0
    # the same rows as three records of one playout each: nothing crosses a row
    one = RO.owner_counts_host(hand_records(), 3, 1, 5.5)
    same_counts(tuple(x.reshape((1, 3) + x.shape[1:]).sum(1).astype(np.int32) for x in one), HAND)
    assert one[4].tolist() == [0, 1, 0] and one[3][0, 81] == one[3][1, 162] == one[3][2, 81] == 1
    # komi -0.5: the margin 0 is black's; A's and C's rows win, and C's white stone is no longer the winner's (80 is still B's)
    b, w, a, h, bw = RO.owner_counts_host(hand_records(), 1, 3, -0.5)
    assert bw.tolist() == [3] and a[0, 80] == 1 and a[0, 0] == 2 and np.array_equal(h, HAND_HIST)
    for bad in ((hand_records(), 2, 3), (hand_records(), 0, 3), (hand_records(), 3, 0), (hand_records()[0], 1, 1),
                (hand_records().astype(np.int8), 1, 3), (hand_records(), 1, 3, float("inf")), (hand_records(), 1, 3, float("nan"))):
        with pytest.raises(ValueError):
            RO.owner_counts_host(*bad)


@pytest.fixture(scope="module")
def five_by_seven():
    """Five golden positions late in their games, both colours to move, and the final boards of 7 host playouts of each."""
    gold = golden_records()
    late = [i for i in range(len(gold)) if (gold[i, :81] != 0).sum() > 45]
    recs = gold[late[::max(1, len(late) // 5)][:5]]
    assert len(recs) == 5 and len(set(L.black_to_move(recs).tolist())) == 2
    final = RO._playouts(recs, 7, L.seed_u64(11), rules="host", final=True).final
    return recs, final


def test_the_mirror_is_owner_host_reduced(five_by_seven):
    recs, final = five_by_seven
    own = RO.owner_host(final)
    score = L.area_score_host(final, L.KOMI).astype(np.float32)
    got = RO.owner_counts_host(final, 5, 7)
    same_counts(got, reduced(own, score > 0, 5, 7))
    assert got[3].sum(1).tolist() == [7] * 5 and (got[0] + got[1] <= 7).all() and (got[2] <= got[0] + got[1]).all()
    assert 0 < got[4].sum() < 35                                          # both colours win some
    for komi in (0.0, 7.5, -3.0):
        same_counts(RO.owner_counts_host(final, 5, 7, komi),
                    reduced(own, L.area_score_host(final, komi).astype(np.float32) > 0, 5, 7))


def test_playout_ownership_on_the_host(five_by_seven):
    recs, final = five_by_seven
    o = RO.playout_ownership(recs, 7, 11, rules="host")
    same_counts(tuple(getattr(o, f) for f in COUNTS), RO.owner_counts_host(final, 5, 7))
    value = RO.playout_value(recs, 7, 11, rules="host")
    assert o.value.dtype == np.float32 and np.array_equal(o.value.view(np.int32), value.view(np.int32))
    assert o.n == 7 and o.wins.dtype == np.int32
    assert np.array_equal(o.wins, np.where(L.black_to_move(recs), o.black_wins, 7 - o.black_wins))
    assert np.array_equal(o.value, ((2 * o.wins - 7) / np.float32(7)).astype(np.float32))
    assert np.array_equal(o.mean_owner, (o.black - o.white) / 7.0) and o.mean_owner.dtype == np.float64
    assert np.array_equal(o.mean_margin, (o.hist * np.arange(-81, 82)).sum(1) / 7.0)
    crit = o.criticality()
    pb = (o.black_wins / 7.0)[:, None]
    assert np.array_equal(crit, o.agree / 7.0 - (o.black / 7.0 * pb + o.white / 7.0 * (1 - pb)))
    assert np.abs(crit).max() <= 0.5 + 1e-12 and (np.abs(crit) > 0).any()
    # the board that needs no luck: black captures, owns its 45 points in every playout and wins them all
    o = RO.playout_ownership(three_records()[:1], 3, 5, rules="host")
    assert o.black_wins.tolist() == [3] and o.hist[0, 81 + 9].tolist() == 3 and not o.criticality().any()
    assert np.array_equal(o.black + o.white, np.full((1, 81), 3)) and np.array_equal(o.agree, o.black)
    with pytest.raises(ValueError):
        RO.playout_ownership(recs, 0, 1, rules="host")
    with pytest.raises(ValueError):
        RO.playout_ownership(recs, 2, 1, rules="nowhere")


# ---- 2. the criticality term of the prior -----------------------------------------------------------------------------------------
def test_gamma_0_and_no_criticality_are_todays_prior():
    recs = three_records()
    a = RO.playout_amaf(recs, 4, 3, rules="host")
    o = RO.playout_ownership(recs, 4, 3, rules="host")
    assert np.array_equal(a.value, o.value) and np.array_equal(a.wins, o.wins)        # the same games
    today = RO.amaf_prior(recs, a)
    crit = o.criticality()
    for kw in (dict(criticality=None), dict(criticality=None, gamma=2.0), dict(criticality=crit, gamma=0.0),
               dict(criticality=crit), dict(gamma=1.0)):
        assert np.array_equal(RO.amaf_prior(recs, a, **kw).view(np.int32), today.view(np.int32)), kw
    assert not np.array_equal(RO.amaf_prior(recs, a, criticality=crit, gamma=1.0), today)
    for bad in (-1.0, -1e-9, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            RO.amaf_prior(recs, a, criticality=crit, gamma=bad)
        with pytest.raises(ValueError):
            RO.amaf_prior(recs, a, gamma=bad)
    with pytest.raises(ValueError):
        RO.amaf_prior(recs, a, criticality=crit[:2], gamma=1.0)


def test_gamma_flips_the_top_prior_of_two_points():
    """n = 4, two wins: wbar = 1/2, k = 4.  Point 10: played 4, won 3: q = (3 + 2) / 8 = 0.625.  Point 20: played 4, won 2:
    q = 0.5.  Every other point: q = 0.5.  With criticality 0.25 at 20 and gamma = 1, q_20 = 0.75 > q_10."""
    recs = records([go.Game()])
    played, won = np.zeros((1, 81), np.int32), np.zeros((1, 81), np.int32)
    played[0, [10, 20]] = 4
    won[0, [10, 20]] = 3, 2
    amaf = RO.Amaf(None, np.array([2], np.int32), played, won, 4)
    crit = np.zeros((1, 81))
    crit[0, 20] = 0.25
    assert RO.amaf_prior(recs, amaf)[0].argmax() == 10
    assert RO.amaf_prior(recs, amaf, criticality=crit, gamma=0.25)[0].argmax() == 10          # 0.5625 < 0.625
    p = RO.amaf_prior(recs, amaf, criticality=crit, gamma=1.0)[0]
    assert p.argmax() == 20 and abs(p.sum() - 1) < 1e-6
    want = np.exp((np.where(np.arange(81) == 20, 0.75, np.where(np.arange(81) == 10, 0.625, 0.5)) - 0.75) / 0.1)
    assert np.array_equal(p, (want / want.sum()).astype(np.float32))


# ---- 3. the evaluator and the search ------------------------------------------------------------------------------------------------
def test_playout_evaluator_with_criticality():
    recs = three_records()
    n, seed = 4, 3
    plain = RO.PlayoutEvaluator(None, n, seed=seed, rules="host", prior=1.0)
    assert plain.criticality == 0.0
    p0, v0 = plain(recs, 2)
    ev = RO.PlayoutEvaluator(None, n, seed=seed, rules="host", prior=1.0, criticality=1.5)
    p1, v1 = ev(recs, 2)
    assert np.array_equal(v1.view(np.int32), v0.view(np.int32)) and p1.shape == p0.shape == (2, 81)
    a = RO.playout_amaf(recs[:2], n, seed, rules="host")
    o = RO.playout_ownership(recs[:2], n, seed, rules="host")
    from bokego_amd.selfplay import normalise_like_categorical
    want = normalise_like_categorical(RO.amaf_prior(recs[:2], a, criticality=o.criticality(), gamma=1.5))
    assert np.array_equal(p1.view(np.int32), want.view(np.int32)) and not np.array_equal(p1[1], p0[1])
    # with rave: the same probs and values, and the records of the evaluator without the term
    pr, vr, rec = RO.PlayoutEvaluator(None, n, seed=seed, rules="host", prior=1.0, criticality=1.5, rave=True)(recs, 2)
    _, _, rec0 = RO.PlayoutEvaluator(None, n, seed=seed, rules="host", prior=1.0, rave=True)(recs, 2)
    assert np.array_equal(pr, p1) and np.array_equal(vr, v0)
    assert rec[0] == rec0[0] and all(np.array_equal(x, y) for x, y in zip(rec[1:], rec0[1:]))
    p, v = ev(recs, 0)                                                    # no policy row: nothing to count
    assert p.shape == (0, 81) and np.array_equal(v, v0)
    for bad in (dict(prior=0.0, criticality=1.0), dict(criticality=1.0), dict(prior=1.0, criticality=-1.0),
                dict(prior=1.0, criticality=float("inf")), dict(prior=1.0, criticality=float("nan"))):
        with pytest.raises(ValueError):
            RO.PlayoutEvaluator(None, n, rules="host", **bad)


def test_native_mcts_with_criticality_on_the_host_rules():
    moves = []
    for _ in range(2):
        t = NativeMCTS(Position(), None, None, playout_value=2, playout_prior=1.0, playout_criticality=1, playout_seed=9,
                       playout_rules="host", expand_thresh=1)
        assert t.playout_criticality == 1.0 and t.evaluator.criticality == 1.0 and t.evaluator.policy_engine is None
        t.rollout(40)
        moves.append((t.choose().last_move, t._pool.root_children(0), t._pool.snapshot(0)))
        t.close()
    assert moves[0] == moves[1] and 0 <= moves[0][0] < 81
    plain = NativeMCTS(Position(board=BOARD), None, None, playout_value=2, playout_prior=1.0, playout_rules="host")
    assert plain.playout_criticality == 0.0 and plain.evaluator.criticality == 0.0
    plain.close()
    with pytest.raises(TypeError, match="playout_prior"):
        NativeMCTS(Position(), None, None, playout_value=2, playout_criticality=1, playout_rules="host")
    with pytest.raises(TypeError):
        NativeMCTS(Position(), None, None, playout_criticality=1)
    for bad in (-1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            NativeMCTS(Position(), None, None, playout_value=2, playout_prior=1.0, playout_criticality=bad,
                       playout_rules="host")


def test_command_lines(capsys):
    assert gtp.parse_args([]).playout_criticality == 0.0
    a = gtp.parse_args(["--playout-value", "64", "--playout-prior", "1", "--playout-rave", "4", "--playout-criticality", "0.5"])
    assert (a.playout_value, a.playout_prior, a.playout_rave, a.playout_criticality) == (64, 1.0, 4.0, 0.5)
    for mod in (gtp, match, selfplay):
        assert mod.parse_args([]).playout_criticality == 0.0
        assert mod.parse_args(["--playout-value", "8", "--playout-prior", "0.5", "--playout-criticality", "2"]).playout_criticality == 2.0
        for bad in (["--playout-criticality", "1"], ["--playout-value", "8", "--playout-criticality", "1"],
                    ["--playout-value", "8", "--playout-prior", "1", "--playout-criticality", "-1"],
                    ["--playout-value", "8", "--playout-prior", "1", "--playout-criticality", "inf"],
                    ["--playout-value", "8", "--playout-prior", "1", "--playout-criticality", "nan"],
                    ["--playout-value", "8", "--playout-prior", "1", "--playout-criticality"]):
            with pytest.raises(SystemExit):
                mod.parse_args(bad)
    assert RO._parse(["--sgf", "g.sgf", "--random", "--ownership"]).ownership
    assert not RO._parse(["--sgf", "g.sgf", "--random"]).ownership
    for bad in (["--sgf", "g.sgf", "--ownership"], ["--sgf", "g.sgf", "--random", "--amaf", "--ownership"],
                ["--sgf", "g.sgf", "-p", "x.bkw", "--ownership"]):
        with pytest.raises(SystemExit):
            RO._parse(bad)
    capsys.readouterr()


# ---- 4. the net-free GTP engine scores by playouts -----------------------------------------------------------------------------------
# Black owns the left five columns with eyes in two corners (0 and 72), white the right four with eyes at 43 and 79, and one
# white stone stands at 37 inside black's wall: its three liberties 28, 36 and 46 are nobody's eye, so both sides play there
# until it is captured, and the four points have no room for two eyes.  Every playout ends with black 45, white 36.
DEAD = "".join([".XXXXOOOO"] + ["XXXXXOOOO"] * 2 + ["X.XXXOOOO", ".OXXXOO.O", "X.XXXOOOO"] + ["XXXXXOOOO"] * 2 + [".XXXXOO.O"])


def test_gtp_scores_by_playouts_without_a_net():
    g = gtp.NativeGTP(Position(board=DEAD), None, None, no_sim=True, time_lim=None, n_rollouts=4, playout_value=2,
                      playout_prior=1.0, playout_rules="host", rollout_score=6, rollout_seed=13)
    assert "final_status_list" in g.commands and g.policy_net is None
    g.running = True
    o = RO.playout_ownership(records([go.Game(DEAD)]), 6, 13, rules="host")
    mean = o.mean_owner[0]
    score = float((mean > 0).sum()) - (float((mean < 0).sum()) + 5.5)
    board = np.frombuffer(DEAD.encode(), np.uint8)
    status = {}
    for s in np.nonzero(board != ord("."))[0].tolist():
        sign = 1.0 if board[s] == ord("X") else -1.0
        status[s] = "seki" if abs(mean[s]) < RO.SEKI_THRESHOLD else "alive" if mean[s] * sign > 0 else "dead"
    assert g.send("final_score") == ("= 0\n\n" if abs(score) < 1e-4 else f"= B+{score}\n\n" if score > 0 else f"= W+{-score}\n\n")
    for word in ("alive", "dead", "seki"):
        want = " ".join(go.unsquash([s for s in sorted(status) if status[s] == word]))
        assert g.send("final_status_list " + word) == f"= {want}\n\n", word
    assert go.unsquash(37) in g.send("final_status_list dead").split()    # the stone in the wall
    g.send("komi 0.5")
    o = RO.playout_ownership(records([go.Game(DEAD)]), 6, 13, rules="host", komi=0.5)
    score = float((o.mean_owner[0] > 0).sum()) - (float((o.mean_owner[0] < 0).sum()) + 0.5)
    assert g.send("final_score") == f"= B+{score}\n\n" and score == 8.5
    g.close()
    # without --rollout-score: the board as it stands, and no status command
    g = gtp.NativeGTP(Position(board=DEAD), None, None, no_sim=True, time_lim=None, n_rollouts=4, playout_value=2,
                      playout_prior=1.0, playout_rules="host")
    g.running = True
    assert g.send("final_status_list dead").startswith("? unknown command")
    stands = g.root.score()                                               # the board as it stands: the white stone is not dead
    assert stands != 3.5 and g.send("final_score") == (f"= B+{stands}\n\n" if stands > 0 else f"= W+{-stands}\n\n")
    g.close()
    r = RO.ownership_score([go.Game(DEAD)], 6, 13, rules="host")[0]
    assert r.stones("dead") == [37] and r.stones("seki") == [] and r.score == 3.5 and r.black_win == 1.0
    assert r.mean_score == 9 - 5.5 and np.array_equal(r.mean_owner, np.where(np.arange(81) % 9 < 5, 1.0, -1.0))


# ---- 5. header, library, Makefile, kernel ---------------------------------------------------------------------------------------
def test_header_binding_and_build_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_owner_counts\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*float\s+komi\s*,\s*int32_t\s*\*\s*black\s*,\s*int32_t\s*\*\s*white\s*,\s*int32_t\s*\*\s*agree\s*,"
                     r"\s*int32_t\s*\*\s*hist\s*,\s*int32_t\s*\*\s*black_wins\s*,\s*void\s*\*\s*stream\s*\)", code)
    comment = re.sub(r"\s*\n \*\s*", " ", src[:src.index("int bkt_owner_counts")].rsplit("/*", 1)[1])
    for phrase in ("exactly the owner bkt_area_score defines", "((float)B - ((float)W + komi)) > 0", "d = B - W",
                   "black[r * 81 + s] += (own[s] == +1)", "white[r * 81 + s] += (own[s] == -1)",
                   "agree[r * 81 + s] += (own[s] == +1 && bw) || (own[s] == -1 && !bw)", "hist[r * 163 + d + 81] += 1",
                   "black_wins[r] += bw", "read only", "BKT_MAX_SAMPLE_ROWS", "komi must be finite", "BKT_ERR_ARG",
                   "nothing written", "Integers only"):
        assert phrase in comment, phrase
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert T.SYMBOLS["bkt_owner_counts"] == (I, [P, I, I, F, P, P, P, P, P, P]) and callable(T.owner_counts)
    for name in ("Ownership", "owner_counts_host", "playout_ownership"):
        assert name in RO.__all__
    assert all(hasattr(RO, name) for name in RO.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_owner_counts
    make = open(os.path.join(CSRC, "Makefile")).read()
    (line,) = [l for l in make.splitlines() if l.startswith("\t") and "-o $@" in l and "bk_playout_pat.hip" in l]
    words = line.split()
    assert "bk_playout_owner.hip" in words and words.index("bk_playout_owner.hip") < words.index("-shared")
    assert "-shared bk_train.hip bk_train_bf16.hip bk_playout_pat.hip -o" in line
    (rule,) = [l for l in make.splitlines() if l.startswith("$(TRAIN_OUT):")]
    assert "bk_playout_owner.hip" in rule.split()
    for name in ("bk_playout.hip", "bk_playout_mc.hip", "bk_playout_pat.hip", "bk_playout_tac.hip", "bk_playout_amaf.hip",
                 "bk_playout_rave.hip"):
        assert "bk_playout_owner" not in open(os.path.join(CSRC, name)).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_builds_alone_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_owner.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    assert len(blocks) == 1 and "owner_counts_kernel" in blocks[0].split()[0], [b.split()[0] for b in blocks]
    field = lambda pat: int(re.search(pat + r": (\d+)", blocks[0]).group(1))  # noqa: E731
    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field(r"SGPRs Spill") == 0 and field(r"VGPRs Spill") == 0, blocks[0]
    # four ballot buffers of 8 words, the seats' partial counts [3][3][81], their histograms [3][163] and win counters [3]
    assert field(r"LDS Size \[bytes/block\]") == 4 * 8 * 4 + 3 * 3 * 81 * 4 + 3 * 163 * 4 + 3 * 4 == 5012, blocks[0]
    assert field(r" VGPRs") <= 64, blocks[0]

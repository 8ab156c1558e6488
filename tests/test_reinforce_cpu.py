"""CPU: the REINFORCE learner's host parts (bokego_amd/reinforce.py) -- Philox, the sampler mirror, the legal plane, the
pool, the loss, the statistics file and the command line."""
import json
import os

import numpy as np
import pytest
import torch

import sampler_cases as SC
from bokego_amd import go
from bokego_amd import reinforce as R
from conftest import GOLDEN


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox_known_answers(ctr, key, want):
    assert R.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32)).tolist() == want


def test_philox_broadcasts_over_counters():
    c = R.counters(np.arange(5), 3, 1, 2).view(np.uint32)
    many = R.philox4x32_10(c, R.seed_key(7))
    for i in range(5):
        assert np.array_equal(many[i], R.philox4x32_10(c[i], R.seed_key(7)))
    assert len({tuple(r) for r in many.tolist()}) == 5


def test_uniform_mapping_and_seed_key():
    x0 = np.array([0, 255, 256, 0xffffffff], np.uint32)
    assert R.uniform(x0).tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert R.seed_key(0x0123456789abcdef).tolist() == [0x89abcdef, 0x01234567]
    assert R.seed_key(-1).tolist() == [0xffffffff, 0xffffffff]


def test_counters_words():
    c = R.counters([0, 5, 4095], 70, 63, 2 ** 32 - 1)
    assert c.dtype == np.int32 and c.shape == (3, 4)
    assert c.view(np.uint32).tolist() == [[0, 70, 63, 2 ** 32 - 1], [5, 70, 63, 2 ** 32 - 1], [4095, 70, 63, 2 ** 32 - 1]]


# ---- the sampler mirror ------------------------------------------------------------------------------------------------
def _row(hot, value=3.0):
    x = np.zeros(81)
    x[hot] = value
    return x


def test_sampler_keeps_a_legal_sample():
    x = np.log(np.full(81, 1.0 / 81))
    legal = np.ones(81, bool)
    for i in (0, 17, 40, 80):
        u = (i + 0.5) / 81
        mv, lp = R.sample_host(x[None], legal[None], [u])
        assert mv.tolist() == [i] and abs(lp[0] - np.log(1 / 81)) < 1e-12


def test_sampler_boundaries_are_inclusive_prefixes():
    x = np.log(np.array([0.25, 0.25, 0.5] + [1e-300] * 78))
    legal = np.ones((1, 81), bool)
    assert R.sample_host(x[None], legal, [0.0])[0][0] == 0
    assert R.sample_host(x[None], legal, [0.25])[0][0] == 1     # prefix 0.25 does not exceed u * S = 0.25
    assert R.sample_host(x[None], legal, [0.5])[0][0] == 2
    assert R.sample_host(x[None], legal, [1 - 2 ** -24])[0][0] == 2


def test_sampler_illegal_sample_takes_the_best_legal_point():
    x = _row(10, 50.0)                              # the sample is 10 for any u
    x[30] = x[60] = 2.0                             # a tie: the lowest index wins
    x[70] = 1.0
    legal = np.zeros(81, bool)
    legal[[30, 60, 70]] = True
    mv, lp = R.sample_host(x[None], legal[None], [0.3])
    assert mv.tolist() == [30]
    want = 2.0 - 50.0 - np.log(np.exp(0.0) + 2 * np.exp(-48.0) + np.exp(-49.0) + 77 * np.exp(-50.0))
    assert abs(lp[0] - want) < 1e-12


def test_sampler_no_legal_point():
    mv, lp = R.sample_host(np.zeros((2, 81)), np.zeros((2, 81), bool), [0.1, 0.9])
    assert mv.tolist() == [-1, -1] and lp.tolist() == [0.0, 0.0]


def test_cdf_margin():
    x = np.log(np.full((1, 81), 1.0 / 81))
    assert abs(R.cdf_margin(x, [1 / 81 + 1e-7])[0] - 1e-7) < 1e-12


# ---- the mirror at the float edges (sampler_cases.py: the kernel meets the same rows in test_gpu_reinforce.py) ------------
def test_indicator_formula_agrees_with_the_mirror():
    """Family A's closed form (the float32 threshold, j = floor(thr)) against the float64 CDF wherever u is not within
    1e-5 of a boundary; the GPU test then holds the kernel to the closed form on every row."""
    x, sup, rs = SC.indicator_rows()
    _, x0 = SC.draws(len(rs))
    want, wlp = SC.indicator_moves(sup, rs, x0)
    u = R.uniform(x0)
    far_rows = 0
    for i, s in enumerate(sup):
        a, b = i * SC.DRAWS_A, (i + 1) * SC.DRAWS_A
        lg = np.repeat(x[i:i + 1], SC.DRAWS_A, 0)
        mv, lp = R.sample_host(lg, np.ones((SC.DRAWS_A, 81), bool), u[a:b])
        far = R.cdf_margin(lg, u[a:b]) >= 1e-5
        far_rows += int(far.sum())
        assert np.array_equal(mv[far], want[a:b][far]), s
        assert np.isin(want[a:b], s).all() and np.abs(lp - wlp[a:b]).max() <= 1e-12
    assert far_rows >= 0.995 * len(rs)
    assert [len(s) for s in sup[:10]] == [1, 1, 1, 1, 2, 2, 64, 17, 81, 27] and len(sup) == 74


def test_replacement_cases_on_the_mirror():
    x, legal, want, names = SC.replacement_rows()
    _, x0 = SC.draws(len(x))
    assert ((x0 >> 8) > 0).all()                                # the premise of family B: then the sample is s for every u
    mv, lp = R.sample_host(x, legal, R.uniform(x0))
    assert mv.tolist() == want.tolist(), [n for n, a, b in zip(names, mv, want) if a != b][:3]
    assert np.array_equal(SC.contract(x, legal)[0], want)       # the cases expect what the plain loop gives
    sampled = np.argmax(x, 1)
    assert set(sampled.tolist()) == set(SC.SAMPLED) and not legal[np.arange(len(x)), sampled].any()
    assert np.isfinite(lp).all()


def test_degenerate_rows_on_the_mirror():
    x, legal, names = SC.degenerate_rows()
    want, deg = SC.contract(x, legal)
    assert np.array_equal(R.degenerate_rows(x), deg)
    for u in (0.0, 0.3, 1 - 2.0 ** -24):                        # no draw: the move is the same for every u
        with np.errstate(all="raise"):                          # and the mirror computes nothing undefined on the way
            mv, lp = R.sample_host(x, legal, np.full(len(x), u))
        assert mv.tolist() == want.tolist(), [n for n, a, b in zip(names, mv, want) if a != b][:3]
        assert np.array_equal(np.isnan(lp), deg), [n for n, a, b in zip(names, np.isnan(lp), deg) if a != b][:3]
        assert (lp[(mv == -1) & ~deg] == 0.0).all()
    by = {n: (int(m), bool(d)) for n, m, d in zip(names, want, deg)}
    assert by["all NaN; point 0 legal"] == (0, True) and by["all NaN; point 0 illegal"] == (7, True)
    assert by["all NaN; no legal point"] == (-1, True)
    assert by["all -inf; point 0 illegal"] == (7, True)
    assert by["one NaN at the legal point 40; point 0 illegal"][1] and by["+inf at the legal point 64; point 0 legal"] == (64, True)
    assert by["NaN at exactly the legal points; point 0 illegal"] == (7, True)
    assert by["NaN at exactly the legal points; no legal point"] == (-1, False)
    assert by["legal logits all -inf among finite illegal ones; point 0 illegal"] == (7, False)
    assert by["legal logits all -inf among finite illegal ones; point 0 legal"] == (0, False)


def test_mirror_takes_the_lowest_legal_index_when_every_legal_logit_is_minus_inf():
    x = np.zeros((2, 81))
    legal = np.zeros((2, 81), bool)
    legal[:, [33, 50]] = True
    x[:, [33, 50]] = -np.inf
    x[1, 0] = np.nan                                            # the same set on a degenerate row
    mv, lp = R.sample_host(x, legal, [0.2, 0.7])
    assert mv.tolist() == [33, 33] and lp[0] == -np.inf and np.isnan(lp[1])


def test_mirror_is_unchanged_on_ordinary_rows():
    """An ordinary row's -inf entries have no mass and are never drawn; the draw is the float64 CDF's as before."""
    with np.errstate(divide="ignore"):
        x = np.log(np.array([0.25, 0.0, 0.25, 0.5] + [0.0] * 77))
    legal = np.ones((1, 81), bool)
    for u, want in ((0.0, 0), (0.25, 2), (0.49, 2), (0.5, 3), (1 - 2.0 ** -24, 3)):
        mv, lp = R.sample_host(x[None], legal, [u])
        assert mv[0] == want and abs(lp[0] - x[want]) < 1e-12


# ---- the legal plane -------------------------------------------------------------------------------------------------
def test_plane5_is_is_legal_along_recorded_playouts():
    rec = json.load(open(os.path.join(GOLDEN, "playouts.json")))
    games = rec["moves"][:40]
    n = 0
    for moves in games:
        g = go.Game()
        for mv in moves:
            plane = g.features_u8()[R.LEGAL_PLANE].reshape(81)
            assert [bool(v) for v in plane] == [g.is_legal(i) for i in range(81)]
            n += 1
            if mv == go.PASS:
                g.play_pass()
            else:
                g.play_move(mv)
    assert n > 1000


def test_batch_features_of_records_match_features_u8():
    """the call the playout driver makes: bk_features_batch_u8 over contiguous bk_pos records"""
    rng = np.random.default_rng(3)
    games = [go.Game() for _ in range(8)]
    for ply in range(30):
        recs = np.stack([np.frombuffer(bytes(g._pos), np.uint8) for g in games])
        out = np.empty((8, 27, 9, 9), np.uint8)
        go.golib().bk_features_batch_u8(recs.ctypes.data, 8, R.POS_BYTES, out.ctypes.data, 0)
        for i, g in enumerate(games):
            assert np.array_equal(out[i], g.features_u8())
            legal = g.get_legal_moves()
            if legal:
                g.play_move(int(rng.choice(legal)))


# ---- the pool ----------------------------------------------------------------------------------------------------------
def _touch(d, *names):
    for n in names:
        open(os.path.join(d, n), "wb").close()


def test_pool_numbering(tmp_path):
    _touch(tmp_path, "policy_0.bkw", "policy_1.pt", "policy_2.pt", "value_3.pt", "policy_x.pt", "notes.txt")
    pool = R.policy_pool(str(tmp_path))
    assert sorted(pool) == [0, 1, 2] and pool[0].endswith("policy_0.bkw")
    assert R.learner_id(pool) == 2
    assert R.choose_opponent(pool, 2, seed=1, epoch=2) == 0
    _touch(tmp_path, "policy_0.pt")
    assert R.policy_pool(str(tmp_path))[0].endswith("policy_0.pt")


def test_opponent_without_policy_0_is_a_seeded_choice(tmp_path):
    pool = {1: "a", 2: "b", 3: "c"}
    picks = [R.choose_opponent(pool, 3, seed=s, epoch=3) for s in range(40)]
    assert set(picks) == {1, 2, 3}
    assert picks == [R.choose_opponent(pool, 3, seed=s, epoch=3) for s in range(40)]
    assert R.choose_opponent({0: "z", 1: "a"}, 1, seed=0, epoch=1, opponent="1") == 1
    assert R.choose_opponent({0: "z", 1: "a", 2: "b"}, 2, 5, 2, opponent="random") in (0, 1, 2)
    with pytest.raises(FileNotFoundError):
        R.choose_opponent(pool, 3, 0, 3, opponent="7")


def test_missing_learner_and_empty_pool(tmp_path):
    with pytest.raises(FileNotFoundError):
        R.learner_id(R.policy_pool(str(tmp_path)), str(tmp_path))
    _touch(tmp_path, "policy_1.pt", "policy_3.pt")          # two policies: n = 1 exists
    assert R.learner_id(R.policy_pool(str(tmp_path))) == 1
    os.remove(os.path.join(tmp_path, "policy_1.pt"))
    with pytest.raises(FileNotFoundError):
        R.learner_id(R.policy_pool(str(tmp_path)))          # one policy: n = 0, and there is no policy_0


# ---- the loss ----------------------------------------------------------------------------------------------------------
def test_loss_sums_every_game_of_the_batch():
    logp = torch.tensor([-1.0, -2.0, -0.5, -3.0, -0.25, -1.5], dtype=torch.float64)
    row_game = torch.tensor([0, 0, 1, 1, 2, 2])
    rewards = torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)
    b = 3
    got = R.reinforce_loss(logp, row_game, rewards, b).item()
    want = (1 * (1.0 + 2.0) - 1 * (0.5 + 3.0) + 1 * (0.25 + 1.5)) / 3
    assert abs(got - want) < 1e-12
    # the reference resets the loss per game and steps on the last game only (selfplay.py:90, 116-117)
    reference_form = rewards[2].item() * (0.25 + 1.5) / b
    assert abs(got - reference_form) > 0.1


def test_loss_gradient_points_along_the_reward():
    logp = torch.tensor([-1.0, -2.0], requires_grad=True)
    R.reinforce_loss(logp, torch.tensor([0, 1]), torch.tensor([1.0, -1.0]), 2).backward()
    assert logp.grad.tolist() == [-0.5, 0.5]        # a descent step raises log pi of the won game, lowers the lost one


# ---- statistics and the command line -----------------------------------------------------------------------------------
def test_stats_lines_format():
    assert R.stats_lines(3, 0, 16, 64, [9, 7, 16, 0]) == ["Policy 3 vs. Policy 0", "Batch Size: 16, Iterations: 64",
                                                          "9,7,16,0"]


@pytest.mark.parametrize("argv", [["-b", "0"], ["-n", "0"], ["-e", "0"], ["--workers", "0"], ["--opponent", "x1"],
                                  ["--seed", "-1"], ["-b", "4096", "--workers", "17"], ["-e", "one"]])
def test_cli_argument_errors(tmp_path, argv):
    with pytest.raises(SystemExit) as e:
        R._parse(["-w", str(tmp_path)] + argv)
    assert e.value.code == 2


def test_cli_defaults_and_missing_dir(tmp_path):
    a = R._parse(["-w", str(tmp_path)])
    assert (a.e, a.n, a.b, a.workers, a.lr, a.seed, a.opponent) == (1, 64, 16, 16, 1e-5, 0, None)
    with pytest.raises(SystemExit):
        R._parse(["-w", str(tmp_path / "nowhere")])


def test_cli_empty_pool_is_an_error(tmp_path):
    with pytest.raises(FileNotFoundError):
        R.main(["-w", str(tmp_path)])

"""-m gpu: the REINFORCE learner on the MI355X (bkt_bn_relu_eval_backward, bkt_sample_moves, bokego_amd/reinforce.py)
against float64 torch on the CPU, the float64 host mirrors and go.Game."""
import ctypes
import math
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampler_cases as SC
from bokego_amd import _trainlib as T
from bokego_amd import go, lockstep, nnet, train
from bokego_amd import reinforce as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CONV = (0, 3, 6, 9, 12, 15, 18)
DEV = torch.device("cuda", 0)


def _seeded(shape, seed, zero_frac=0.2):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    a[torch.rand(shape, generator=g) < zero_frac] = 0
    return a.float()


def _rel_max(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


@pytest.fixture(scope="module")
def golden():
    feats = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"].astype(np.uint8)
    return feats, train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))


# ---- eval-mode BatchNorm + ReLU backward --------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17, 560, 4096])
def test_bn_relu_eval_backward_against_float64(B):
    x = _seeded((B, 128, 9, 9), 11 + B, 0.05) * 2 + 0.3
    gamma, beta = _seeded((128,), 1, 0) * 0.5 + 1, _seeded((128,), 2, 0) * 0.2
    rm, rv = _seeded((128,), 3, 0) * 0.5, _seeded((128,), 4, 0).abs() + 0.2
    dy = _seeded((B, 128, 9, 9), 5 + B)
    xg, gg, bg, rmg, rvg, dyg = (t.to(DEV) for t in (x, gamma, beta, rm, rv, dy))
    y = T.bn_relu_eval(xg, gg, bg, rmg, rvg)
    dx, dgamma, dbeta = T.bn_relu_eval_backward(dyg, y, xg, gg, rmg, rvg)

    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    mask = (y > 0).cpu().double()                   # the kernel's ReLU mask (fp32 y), so both differentiate one function
    z = F.batch_norm(xd, rm.double(), rv.double(), gd, bd, training=False, eps=1e-5)
    (z * mask * dy.double()).sum().backward()
    assert _rel_max(dx, xd.grad) <= 1e-5
    assert _rel_max(dgamma, gd.grad) <= 1e-4
    assert _rel_max(dbeta, bd.grad) <= 1e-4

    again = T.bn_relu_eval_backward(dyg, y, xg, gg, rmg, rvg)
    assert all(torch.equal(a, b) for a, b in zip((dx, dgamma, dbeta), again))


# ---- the full REINFORCE gradient through the eval-mode trainable net ------------------------------------------------------
def _ref64_eval(sd, x):
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()
         if "running_" not in k and not k.endswith("num_batches_tracked")}
    h = x.double()
    for l, c in enumerate(CONV):
        h = F.conv2d(h, p[f"conv.{c}.weight"], p[f"conv.{c}.bias"], padding=2 if l == 0 else 1)
        b = f"conv.{c + 1}"
        h = torch.relu(F.batch_norm(h, sd[b + ".running_mean"].double(), sd[b + ".running_var"].double(),
                                    p[b + ".weight"], p[b + ".bias"], training=False, eps=1e-5))
    z = F.conv2d(h, p["conv.21.weight"]) + p["conv.21.bias"]
    return z.reshape(-1, 81), p


def test_reinforce_gradient_against_float64(golden):
    feats, psd = golden
    rng = np.random.default_rng(4)
    R_, b = 200, 6
    x = torch.from_numpy(feats[:R_].astype(np.float32))
    played = torch.from_numpy(rng.integers(0, 81, R_))
    row_game = torch.from_numpy(np.sort(rng.integers(0, b, R_)))
    rewards = torch.tensor([1.0, -1.0, -1.0, 1.0, 1.0, -1.0])

    net = train.TrainablePolicyNet.from_state_dict(psd, device=DEV).eval()
    loss = R.reinforce_loss(R.played_logp(net, x.to(DEV), played.to(DEV)), row_game.to(DEV), rewards.to(DEV), b)
    loss.backward()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    logits, p = _ref64_eval(sd, x)
    rlogp = F.log_softmax(logits, 1).gather(1, played.reshape(-1, 1)).reshape(-1)
    rloss = R.reinforce_loss(rlogp, row_game, rewards.double(), b)
    rloss.backward()
    assert abs(loss.item() - rloss.item()) <= 1e-5 * abs(rloss.item())
    grads = {n: q.grad for n, q in net.named_parameters()}
    assert set(grads) == set(p) and all(g is not None for g in grads.values())
    bad = {n: _rel_max(g, p[n].grad) for n, g in grads.items()}
    assert max(bad.values()) <= 1e-4, bad
    # eval mode froze the running statistics
    assert all(torch.equal(v.cpu(), train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))[k])
               for k, v in net.state_dict().items() if "running_" in k)


def test_eval_mode_without_grad_is_unchanged(golden):
    feats, psd = golden
    net = train.TrainablePolicyNet.from_state_dict(psd, device=DEV).eval()
    x = torch.from_numpy(feats[:64]).to(DEV)
    with torch.no_grad():
        a = net(x)
    b = net(x)
    assert torch.equal(a, b.detach()) and b.requires_grad and not a.requires_grad


# ---- the sampler ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine_logits(golden):
    feats, psd = golden
    eng = R.policy_engine(psd, 0, 1024)
    try:
        lg = eng.eval(feats, logits=True, probs=False, value=False)["logits"]
    finally:
        eng.close()
    return feats, lg


def _draws(n, seed):
    c = R.counters(np.arange(n), 0, 5, 9)
    return c, R.uniform(R.philox4x32_10(c.view(np.uint32), R.seed_key(seed))[:, 0])


def test_sampler_matches_the_host_mirror(engine_logits):
    feats, lg = engine_logits
    reps = 200
    n = len(feats) * reps                                         # 107 200 rows
    seed = 0xC0FFEE12345678
    rows = np.arange(n) % len(feats)
    c, u = _draws(n, seed)
    d_lg = torch.from_numpy(lg).to(DEV)[torch.from_numpy(rows).to(DEV)].contiguous()
    d_pl = torch.from_numpy(feats).to(DEV)[torch.from_numpy(rows).to(DEV)].contiguous()
    moves, logp = T.sample_moves(d_lg, d_pl, seed, torch.from_numpy(c).to(DEV))
    moves, logp = moves.cpu().numpy(), logp.cpu().numpy()
    legal = feats[rows, R.LEGAL_PLANE].reshape(n, 81) != 0
    want, wlogp = R.sample_host(lg[rows], legal, u)
    near = R.cdf_margin(lg[rows], u) < 1e-5
    diff = moves != want
    assert near.mean() <= 0.005
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:10]
    same = ~diff
    assert np.abs(logp[same] - wlogp[same]).max() <= 1e-5
    ok = moves >= 0
    assert (legal[np.arange(n)[ok], moves[ok]]).all() and (legal[~ok] == 0).all()
    again = T.sample_moves(d_lg, d_pl, seed, torch.from_numpy(c).to(DEV))[0].cpu().numpy()
    assert np.array_equal(again, moves)


def test_sampler_forced_illegal_and_no_legal_point():
    x = np.zeros((3, 81), np.float32)
    x[:, 10] = 50.0
    x[:, 30] = x[:, 60] = 2.0
    planes = np.zeros((3, 27, 9, 9), np.uint8)
    pl = planes[:, R.LEGAL_PLANE].reshape(3, 81)
    pl[0, [30, 60, 70]] = 1                                      # 10 is sampled whatever u is, and it is illegal
    pl[1, 10] = 1                                                # legal: kept
    c = R.counters([0, 1, 2], 0, 0, 0)
    moves, logp = T.sample_moves(torch.from_numpy(x).to(DEV), torch.from_numpy(planes).to(DEV), 3,
                                 torch.from_numpy(c).to(DEV))
    assert moves.cpu().tolist() == [30, 10, -1]
    _, wl = R.sample_host(x, pl != 0, [0.5] * 3)
    assert abs(logp[0].item() - wl[0]) <= 1e-5 and abs(logp[1].item() - wl[1]) <= 1e-5 and logp[2].item() == 0.0


def _chi2_sf(stat, df):
    """upper tail of chi^2(df), Wilson-Hilferty"""
    z = ((stat / df) ** (1 / 3) - (1 - 2 / (9 * df))) / math.sqrt(2 / (9 * df))
    return 0.5 * math.erfc(z / math.sqrt(2))


def test_sampler_chi_square(engine_logits):
    feats, lg = engine_logits
    n = 2 ** 20
    row = lg[200].astype(np.float64)
    planes = np.repeat(feats[200:201], 1, 0).copy()
    planes[:, R.LEGAL_PLANE] = 1                                # every point legal: draws follow softmax exactly
    d_pl = torch.from_numpy(planes).to(DEV).expand(n, 27, 9, 9).contiguous()
    d_lg = torch.from_numpy(lg[200:201]).to(DEV).expand(n, 81).contiguous()
    c = R.counters(np.arange(n), 0, 0, 0)
    moves = T.sample_moves(d_lg, d_pl, 2024, torch.from_numpy(c).to(DEV))[0].cpu().numpy()
    p = np.exp(row - row.max())
    p /= p.sum()
    obs = np.bincount(moves, minlength=81).astype(np.float64)
    exp = n * p
    big = exp >= 5
    o = np.append(obs[big], obs[~big].sum())
    e = np.append(exp[big], exp[~big].sum())
    if e[-1] < 5:
        o, e = o[:-1], e[:-1]
        o[-1] += obs[~big].sum()
        e[-1] += exp[~big].sum()
    stat = float(((o - e) ** 2 / e).sum())
    assert _chi2_sf(stat, len(o) - 1) > 1e-6, stat


# ---- the sampler at the float edges (sampler_cases.py; test_reinforce_cpu.py holds the mirror to the same rows) -----------
def _sample_checked(x, mask, c):
    """bkt_sample_moves of logits x (numpy f32 [n,81], or a device tensor) with the legal plane = mask (numpy bool [n,81],
    or None: every point), counters c -> (moves, logp) as numpy.  On the way: a second call and one call of
    bkt_sample_moves_masked with mask_stride 81 give the same bits, and every move is a point of its row's set, -1
    exactly where the set is empty."""
    d_lg = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    n = len(d_lg)
    d_mask = (torch.ones((n, 81), dtype=torch.uint8, device=DEV) if mask is None else
              torch.from_numpy(mask.astype(np.uint8)).to(DEV))
    planes = torch.zeros((n, 27, 81), dtype=torch.uint8, device=DEV)
    planes[:, R.LEGAL_PLANE] = d_mask
    planes, d_c = planes.view(n, 27, 9, 9), torch.from_numpy(c).to(DEV)
    mv, lp = T.sample_moves(d_lg, planes, SC.SEED, d_c)
    for amv, alp in (T.sample_moves(d_lg, planes, SC.SEED, d_c), T.sample_moves_masked(d_lg, d_mask, SC.SEED, d_c)):
        assert torch.equal(amv, mv) and torch.equal(alp.view(torch.int32), lp.view(torch.int32))
    mv, lp = mv.cpu().numpy(), lp.cpu().numpy()
    assert ((mv >= -1) & (mv <= 80)).all(), mv[(mv < -1) | (mv > 80)][:10]
    some = np.ones(n, bool) if mask is None else mask.any(1)
    assert np.array_equal(mv >= 0, some)
    assert mask is None or mask[np.arange(n)[some], mv[some]].all()
    return mv, lp


def test_sampler_indicator_rows_are_exact():
    """Family A.  Logits in {0, -inf}: p is 0 or 1, every prefix an exact integer, S = n, and the threshold has one
    rounding that numpy's float32 reproduces (sampler_cases.indicator_moves), so the move is s_floor(thr) on every one of
    the 74 x 4096 rows, none excused: the prefix scan inside a register, across the lanes, and across the split between
    points 63 and 64."""
    x, sup, rs = SC.indicator_rows()
    c, x0 = SC.draws(len(rs))
    want, wlp = SC.indicator_moves(sup, rs, x0)
    d_lg = torch.from_numpy(x).to(DEV)[torch.from_numpy(rs).to(DEV)].contiguous()
    mv, lp = _sample_checked(d_lg, None, c)
    bad = np.nonzero(mv != want)[0]
    assert len(bad) == 0, [(sup[rs[r]].tolist(), int(x0[r]), int(mv[r]), int(want[r])) for r in bad[:3]]
    assert np.abs(lp - wlp).max() <= 1e-6


def test_sampler_replacement_tie_breaks():
    """Family B.  The sample is one illegal point for every draw (k > 0 asserted), below and above the split; the move
    is the case's: ties inside a lane, across lanes, against the lane order, and a best point at 63, 64 or 80."""
    x, legal, want, names = SC.replacement_rows()
    c, x0 = SC.draws(len(x))
    assert ((x0 >> 8) > 0).all()
    mv, lp = _sample_checked(x, legal, c)
    assert mv.tolist() == want.tolist(), [(n, int(a), int(b)) for n, a, b in zip(names, mv, want) if a != b][:3]
    assert np.abs(lp - R.sample_host(x, legal, R.uniform(x0))[1]).max() <= 1e-5


@pytest.mark.parametrize("s", SC.SPREADS)
def test_sampler_spreads(s):
    """Family C.  x = s * z on 40 000 rows, every point legal, by the rule of the mirror test: at most 0.5 % of the rows
    have u within 1e-5 of a CDF boundary, and no row outside them differs.  logp within 1e-5 + 2^-22 * max |x| (the second
    term: the one rounding of x[mv] - m, half an ulp of a value up to 2 * max |x|)."""
    x = SC.spread_rows(s)
    c, x0 = SC.draws(len(x))
    u = R.uniform(x0)
    mv, lp = _sample_checked(x, None, c)
    want, wlp = R.sample_host(x, np.ones(x.shape, bool), u)
    near = R.cdf_margin(x, u) < 1e-5
    diff = mv != want
    same = ~diff
    err = np.abs(lp[same] - wlp[same]) / (1e-5 + 2.0 ** -22 * np.abs(x).max(1)[same])
    print(f"spread {s}: near share {100 * near.mean():.4f} %, differing rows {int(diff.sum())}, "
          f"largest logp error / tolerance {err.max():.3f}")
    assert near.mean() <= 0.005
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:10]
    assert err.max() <= 1.0


def test_sampler_degenerate_rows():
    """Family D.  Rows with a NaN, a +inf or nothing but -inf, and their ordinary neighbours, each with point 0 legal,
    illegal and with no legal point: the move is the contract's (sampler_cases.contract, a plain loop) and the
    mirror's, logp is NaN exactly on the degenerate rows, 0 on an ordinary row without a legal point."""
    x, legal, names = SC.degenerate_rows()
    want, deg = SC.contract(x, legal)
    c, x0 = SC.draws(len(x))
    mv, lp = _sample_checked(x, legal, c)
    hmv, hlp = R.sample_host(x, legal, R.uniform(x0))
    assert mv.tolist() == want.tolist(), [(n, int(a), int(b)) for n, a, b in zip(names, mv, want) if a != b][:3]
    assert mv.tolist() == hmv.tolist()
    assert np.array_equal(np.isnan(lp), deg), [n for n, a, b in zip(names, np.isnan(lp), deg) if a != b][:3]
    assert (lp[(mv == -1) & ~deg] == 0.0).all()
    inf = np.isinf(hlp)                                          # an ordinary row whose move has the logit -inf
    assert np.array_equal(lp[inf], hlp[inf].astype(np.float32)) and inf.any()
    fin = ~deg & ~inf
    assert np.abs(lp[fin] - hlp[fin]).max() <= 1e-5


def test_sampler_degenerate_rows_write_only_their_outputs():
    """The C entry points on family D with 64 sentinel elements before and behind moves and logp: untouched, and the
    elements between them are what the binding returns."""
    x, legal, _ = SC.degenerate_rows()
    n, guard = len(x), 64
    c, _ = SC.draws(n)
    d_lg, d_c = torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV)
    d_mask = torch.from_numpy(legal.astype(np.uint8)).to(DEV)
    want_mv, want_lp = T.sample_moves_masked(d_lg, d_mask, SC.SEED, d_c)
    planes = torch.zeros((n, 27, 81), dtype=torch.uint8, device=DEV)
    planes[:, R.LEGAL_PLANE] = d_mask
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    lib = T.load()
    for call in (lambda m, l: lib.bkt_sample_moves_masked(d_lg.data_ptr(), d_mask.data_ptr(), 81, n, SC.SEED,
                                                          d_c.data_ptr(), m, l, stream),
                 lambda m, l: lib.bkt_sample_moves(d_lg.data_ptr(), planes.data_ptr(), n, SC.SEED, d_c.data_ptr(), m, l,
                                                   stream)):
        moves = torch.full((n + 2 * guard,), -77, dtype=torch.int32, device=DEV)
        logp = torch.full((n + 2 * guard,), -77.0, dtype=torch.float32, device=DEV)
        assert call(moves.data_ptr() + 4 * guard, logp.data_ptr() + 4 * guard) == 0
        torch.cuda.synchronize(DEV)
        for buf in (moves, logp):
            assert (buf[:guard] == -77).all().item() and (buf[-guard:] == -77).all().item()
        assert torch.equal(moves[guard:-guard], want_mv)
        assert torch.equal(logp[guard:-guard].view(torch.int32), want_lp.view(torch.int32))


def test_play_games_reports_logits_that_are_not_finite(engines, monkeypatch):
    """One row of every ply's logits poisoned with NaN (row 0: game 0 on its first ply, the learner's): the sampler
    still gives legal moves, so the games run to their end, and play_games raises when the results reach the host."""
    a, b = engines
    real = lockstep.engine_logits

    def poisoned(pairs):
        lg = real(pairs).clone()
        lg[0] = float("nan")
        return lg

    monkeypatch.setattr(lockstep, "engine_logits", poisoned)
    for rules in ("device", "host"):
        with pytest.raises(FloatingPointError, match=r"game 0: the policy's logits are not finite"):
            R.play_games(a, b, 2, 4, seed=7, rules=rules)


# ---- playouts --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(golden):
    _, psd = golden
    other = {k: (v + 0.05 * torch.randn(v.shape, generator=torch.Generator().manual_seed(1), dtype=v.dtype)
                 if v.dtype.is_floating_point and "running_var" not in k else v) for k, v in psd.items()}
    a, b = R.policy_engine(psd, 0, 64), R.policy_engine(other, 0, 64)
    yield a, b
    a.close()
    b.close()


def _replay(moves, length):
    g = go.Game()
    seen = []
    for t in range(length):
        seen.append((g.features_u8(), g.turn))
        assert g.is_legal(int(moves[t])), (t, moves[t])
        g.play_move(int(moves[t]))
    return g, seen


def test_playouts_follow_the_rules(engines):
    a, b = engines
    W, bs = 4, 8
    games = R.play_games(a, b, W, bs, seed=7)
    G = W * bs
    exp_rows, exp_moves, exp_game = [], [], []
    per_ply = {}
    for g in range(G):
        L = int(games.length[g])
        end, seen = _replay(games.moves[g], L)
        assert (games.moves[g, L:] == go.PASS).all()
        assert L == R.POLICY_MAX_TURNS + 1 or not end.get_legal_moves()      # turn > 70, or no legal point
        assert games.black_wins[g] == (end.area_score() > 0)
        assert games.reward[g] == (1.0 if games.black_wins[g] == games.learner_black[g] else -1.0)
        for t, (f, _) in enumerate(seen):
            if games.learner_black[g] == (t % 2 == 0):
                per_ply.setdefault(t, []).append((g, f, int(games.moves[g, t])))
    for t in sorted(per_ply):
        for g, f, mv in per_ply[t]:
            exp_game.append(g)
            exp_rows.append(f)
            exp_moves.append(mv)
    assert games.row_game.tolist() == exp_game
    assert np.array_equal(games.planes.cpu().numpy(), np.stack(exp_rows))
    assert games.played.cpu().tolist() == exp_moves
    assert games.learner_black.tolist() == [(g // bs) % 2 == 0 for g in range(G)]

    again = R.play_games(a, b, W, bs, seed=7)
    assert np.array_equal(again.moves, games.moves) and torch.equal(again.planes, games.planes)
    other = R.play_games(a, b, W, bs, seed=8)
    assert not np.array_equal(other.moves, games.moves)
    later = R.play_games(a, b, W, bs, seed=7, iteration=1)
    assert not np.array_equal(later.moves, games.moves)


def test_learner_logp_matches_the_sampler(engines, golden):
    a, b = engines
    games = R.play_games(a, b, 2, 8, seed=3)
    net = train.TrainablePolicyNet.from_state_dict(golden[1], device=DEV).eval()
    with torch.no_grad():
        lp = R.played_logp(net, games.planes, games.played)
    assert (lp - games.logp).abs().max().item() < 1e-4


# ---- the update ------------------------------------------------------------------------------------------------------
def test_engine_follows_the_trainable_net(golden):
    feats, psd = golden
    net = train.TrainablePolicyNet.from_state_dict(psd, device=DEV).eval()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    eng, opp = R.policy_engine(psd, 0, 256), R.policy_engine(psd, 0, 256)
    try:
        for it in range(2):
            games = R.play_games(eng, opp, 2, 8, seed=11, iteration=it)
            R.update(net, opt, games, 2, 8)
            eng.set_weights(R.engine_weights(net))
            x = torch.from_numpy(feats[:256]).to(DEV)
            with torch.no_grad():
                want = net(x)
            got = eng.eval_device(x, logits=True, probs=False, value=False)["logits"]
            assert (got - want).abs().max().item() < 1e-4
        start = torch.as_tensor(nnet.HipPolicyNet(psd)(feats[:256].astype(np.float32))).cpu()
        assert (want.cpu() - start).abs().max().item() > 1e-3         # the steps moved the policy
    finally:
        eng.close()
        opp.close()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_update_direction(engines, golden, sign):
    a, b = engines
    games = R.play_games(a, b, 2, 8, seed=5)
    net = train.TrainablePolicyNet.from_state_dict(golden[1], device=DEV).eval()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4)
    with torch.no_grad():
        before = R.played_logp(net, games.planes, games.played).mean().item()
    R.update(net, opt, games, 2, 8, reward_override=sign)
    with torch.no_grad():
        after = R.played_logp(net, games.planes, games.played).mean().item()
    assert (after - before) * sign > 0, (before, after)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _pool(d):
    os.makedirs(d)
    shutil.copy(os.path.join(GOLDEN, "policy_19.bkw"), os.path.join(d, "policy_0.bkw"))
    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    g = torch.Generator().manual_seed(3)
    pert = {k: (v + 0.02 * v.abs().mean() * torch.randn(v.shape, generator=g) if k.endswith("weight") else v)
            for k, v in sd.items()}
    torch.save({"model_state_dict": pert}, os.path.join(d, "policy_1.pt"))


def test_end_to_end(tmp_path, capsys):
    runs = []
    for r in range(2):
        d = str(tmp_path / f"pool{r}")
        _pool(d)
        stats = str(tmp_path / f"stats{r}.txt")
        R.main(["-w", d, "-e", "1", "-n", "2", "-b", "4", "--workers", "4", "--seed", "7", "-f", stats])
        lines = open(stats).read().splitlines()
        assert lines[:2] == ["Policy 1 vs. Policy 0", "Batch Size: 4, Iterations: 2"]
        wins = [int(w) for w in lines[2].split(",")]
        assert len(lines) == 3 and len(wins) == 8 and all(0 <= w <= 4 for w in wins)
        ck = torch.load(os.path.join(d, "policy_2.pt"))
        assert set(ck) == {"model_state_dict", "optimizer_state_dict"}
        runs.append((ck, lines))
    capsys.readouterr()
    (a, la), (b, lb) = runs
    assert la == lb
    assert a["model_state_dict"].keys() == b["model_state_dict"].keys()
    assert all(torch.equal(a["model_state_dict"][k], b["model_state_dict"][k]) for k in a["model_state_dict"])
    sa, sb = a["optimizer_state_dict"]["state"], b["optimizer_state_dict"]["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i])
    start = torch.load(str(tmp_path / "pool0" / "policy_1.pt"))["model_state_dict"]
    assert not torch.equal(a["model_state_dict"]["conv.3.weight"], start["conv.3.weight"])
    assert torch.equal(a["model_state_dict"]["conv.4.running_var"], start["conv.4.running_var"])
    hp = nnet.HipPolicyNet(a["model_state_dict"])
    feats = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"][:32].astype(np.float32)
    net = train.TrainablePolicyNet.from_state_dict(a, device=DEV).eval()
    with torch.no_grad():
        want = net(torch.from_numpy(feats).to(DEV)).cpu()
    assert (torch.as_tensor(hp(feats)) - want).abs().max().item() < 1e-4

"""The nets of tests/weight_cases.py and their float64 reference on their own.  No GPU: this is what keeps
test_gpu_weight_domain.py from passing on cases that do not reach what they are named after, on bounds the reference's own
fp32 arithmetic nearly fills, or on an expected fallback count that rounding decides."""
import numpy as np
import pytest

import weight_cases as W

TOL_LOGIT, TOL_VALUE, TOL_PROB = 1e-4, 1e-4, 1e-5      # test_gpu_parity's (that module is marked gpu as a whole)
FALLS_BACK = {"tiny_var_full_w", "huge_fold"}          # A beyond the f16x2 flag: every other case stays on the f16x2 kernel


def _trunk_names(sd):
    return [k for k in sd if k.startswith("conv.")]


def test_the_case_list_is_the_documented_one():
    assert len(W.NAMES) == len(set(W.NAMES)) == 12 and FALLS_BACK < set(W.NAMES)
    x = W.inputs()
    assert x.dtype == np.uint8 and x.shape == (32, 27, 9, 9)
    assert not x[30].any() and (x[31] == 1).all()
    assert W.planes(W.FLOAT_PLANES).dtype == np.float32 and W.planes("neg_gamma").dtype == np.uint8


@pytest.mark.parametrize("name", W.NAMES)
def test_weights_are_what_the_engine_accepts(name):
    """bokego_amd.h: finite, and running_var + eps > 0 -- with the reference's names and shapes"""
    from bokego_amd.bkw import load_bkw
    from conftest import GOLDEN
    import os
    p, v = W.nets(name)
    gp, gv = load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw"))
    for sd, gold in ((p, gp), (v, gv)):
        for k in sd:
            assert np.asarray(gold[k]).size == sd[k].size, k
            assert np.isfinite(sd[k]).all(), k
            if k.endswith("running_var"):
                assert (sd[k].astype(np.float64) + W.EPS > 0).all(), k
    assert set(p) == {k for k in gp if k.startswith("conv.")}
    assert set(v) >= set(_trunk_names(p)) | {"bn.weight", "lin1.weight", "lin_bn.running_var", "lin2.bias"}


@pytest.mark.parametrize("name", W.NAMES)
def test_reference_is_finite_and_well_inside_every_bound(name):
    """The reference's own fp32 evaluation within one third of each bound test_gpu_weight_domain.py applies: the bounds
    leave room for a second fp32 summation order.  A case that fails this is to be changed, never the bound."""
    r = W.reference(name)
    for a in r[:-1]:
        assert np.isfinite(a).all()
    assert np.isfinite(r.A)
    d = W.delta(name, TOL_LOGIT)
    own = W.softmax64(r.lg32)
    fig = {"logits": np.abs(r.lg32 - r.lg64).max() / d,
           "value": np.abs(r.va32 - r.va64).max() / TOL_VALUE,
           "softmax of its own logits": np.abs(r.pr32 - own).max() / TOL_PROB,
           "probs": np.abs(r.pr32 - r.pr64).max() / (d / 2),
           "row sums": np.abs(r.pr32.astype(np.float64).sum(1) - 1).max() / 1e-5}
    print(f"{name}: |lg64|max {np.abs(r.lg64).max():.4g} delta {d:.3g} A {r.A:.4g} share of each bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    assert all(v < 1 / 3 for v in fig.values()), fig
    assert (np.abs(r.va64) <= 1).all()


@pytest.mark.parametrize("name", W.NAMES)
def test_no_case_sits_near_the_f16x2_flag(name):
    """The flag rises at an activation of 4094: a factor of two on either side is kept clear"""
    A = W.reference(name).A
    assert A < W.FLAG_AT / 2 or A > W.FLAG_AT * 2
    assert (A > W.FLAG_AT * 2) == (name in FALLS_BACK)


def _both(name):
    return [(sd, *W.folded(sd)) for sd in W.nets(name)]


def test_neg_gamma():
    p, v = W.nets("neg_gamma")
    for sd, scale, wmax in _both("neg_gamma"):
        assert ((scale < 0).sum(1) == 43).all()                  # every third of 128, in every layer
    assert v["bn.weight"][0] < 0 and (v["lin_bn.weight"] < 0).sum() == 32


def test_zero_gamma():
    for sd, scale, wmax in _both("zero_gamma"):
        assert ((scale == 0).sum(1) == 26).all() and ((wmax == 0).sum(1) == 26).all()


def test_tiny_var():
    for name, zeros, tiny in (("tiny_var_small_w", 8, 8), ("tiny_var_full_w", 4, 0)):
        for sd, scale, wmax in _both(name):
            for c in W.CONV:
                var = sd[f"conv.{c + 1}.running_var"]
                assert var.min() == 0 and (var == 0).sum() == zeros and (var == np.float32(1e-12)).sum() == tiny
            big = np.abs(scale) > 100                            # gamma / sqrt(eps) = 316 * gamma
            assert (big.sum(1) == zeros + tiny).all()
            ratio = wmax.max(1) / wmax.min(1)
            # small_w: the large scales meet weights of 1e-3 and fold to an ordinary layer; full_w: they do not
            assert (ratio < 30).all() if name == "tiny_var_small_w" else (ratio > 300).all()


def test_scale_invariant():
    base_p, base_v, _ = W.base(15)
    for (sd, scale, wmax), b in zip(_both("scale_invariant"), (base_p, base_v)):
        _, bmax = W.folded(b)
        # an ordinary folded net: the base's, but for eps, which weighs more against a variance scaled by 2^-20 ...
        assert (wmax <= bmax * (1 + 2e-5)).all() and (wmax > bmax / 6).all() and (wmax.max(1) / wmax.min(1) < 20).all()
        assert np.isclose(wmax, bmax, rtol=1e-2).mean() > 0.6
        for c in W.CONV:                                         # ... from raw tensors that span 2^+-10 per channel
            raw = np.abs(sd[f"conv.{c}.weight"]).reshape(128, -1).max(1) / np.abs(b[f"conv.{c}.weight"]).reshape(128, -1).max(1)
            assert raw.max() == 1024 and raw.min() == 1 / 1024
            assert sd[f"conv.{c + 1}.running_var"].max() / sd[f"conv.{c + 1}.running_var"].min() > 2.0 ** 30


def test_gamma_range():
    for sd, scale, wmax in _both("gamma_range"):
        assert (wmax.max(1) / wmax.min(1) > 1000).all()          # 2^11 between the channels' scales, less the weights' spread


def test_zero_and_tiny_layer():
    for sd, scale, wmax in _both("zero_layer"):
        assert wmax[3].max() == 0 and (wmax[[0, 1, 2, 4, 5, 6]].max(1) > 0.1).all()
        assert W.f16_exponent(wmax[3].max()) == (0, 0)
    for sd, scale, wmax in _both("tiny_layer"):
        raw, el = W.f16_exponent(wmax[2].max())
        assert raw > 24 and el == 24                             # the upper clamp
        assert 0 < wmax[2].max() < 2.0 ** -20
        assert all(W.f16_exponent(wmax[l].max())[0] in range(-14, 25) for l in (0, 1, 3, 4, 5, 6))


def test_heads():
    r = W.reference("big_heads")
    assert np.abs(r.va64).max() > 1 - 1e-9 and np.abs(r.lg64).max() > 10
    u = W.reference("uniform_policy")
    assert (u.lg64 == 0.25).all() and (u.lg32 == np.float32(0.25)).all()
    g = W.reference("gain3")
    assert np.abs(g.lg64).max() > 150 and g.pr64.min() < 1e-100 and 1000 < g.A < W.FLAG_AT / 2


def test_huge_fold():
    for sd, scale, wmax in _both("huge_fold"):
        layer = wmax.max(1)
        assert (layer[:6] < 1).all() and wmax[6].argmax() == W.HUGE_CHANNEL
        assert 2.0 ** 30.9 < layer[6] < 2.0 ** 31.1
        raw, el = W.f16_exponent(layer[6])
        assert raw < -14 and el == -14                           # the lower clamp ...
        with np.errstate(over="ignore"):
            assert np.isinf(np.float16(layer[6] * 2.0 ** el))    # ... at which the weight is +Inf in fp16
        assert np.sort(wmax[6])[-2] < 1                          # one channel only
    assert 1e5 < np.abs(W.reference("huge_fold").lg64).max() < 1e6
    # every layer of every other case stays inside fp16
    for name in W.NAMES:
        if name != "huge_fold":
            for sd, scale, wmax in _both(name):
                for l in range(7):
                    assert wmax[l].max() * 2.0 ** W.f16_exponent(wmax[l].max())[1] <= 32768


def test_big_planes_reference_is_well_inside_its_bounds():
    """test_gpu_weight_domain.test_float_planes_beyond_fp16_are_redone_in_fp32: the same third of the same bounds"""
    lg64, va64, lg32, va32 = W.big_planes_reference()
    d = TOL_LOGIT * max(1.0, float(np.abs(lg64).max()) / 15.0)
    with np.errstate(over="ignore"):
        assert np.isinf(W.big_planes().astype(np.float16)).any()
    assert np.isfinite(lg64).all() and np.isfinite(lg32).all()
    fig = np.abs(lg32 - lg64).max() / d, np.abs(va32 - va64).max() / TOL_VALUE
    print(f"|lg64|max {np.abs(lg64).max():.4g} delta {d:.3g}; share of each bound: logits {fig[0]:.3f}, value {fig[1]:.3f}")
    assert max(fig) < 1 / 3

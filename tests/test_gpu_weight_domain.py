"""-m gpu: both precisions of the leaf engine on finite nets from the corners of the accepted weight domain, against float64.

The nets, the 32 rows and the reference are tests/weight_cases.py's (tests/test_weight_domain_cpu.py shows on the reference
alone that every case reaches what it is named after, that the reference's own fp32 evaluation fills less than a third of
each bound below, and that no case sits within a factor of two of the f16x2 flag's threshold).  Whatever finite net the
engine accepts, both precisions return the reference's numbers, or f16x2 visibly falls back: with A the largest trunk
activation in float64, A < 2047 means no fallback, A > 8188 exactly one and the fp32 kernel's bits.

Every test makes one engine (the f16x2 side of a case that falls back, run on its own, a second one for the fp32 bits) and
evaluates at most 34 rows.
"""
import os

import numpy as np
import pytest

import weight_cases as W
from conftest import GOLDEN
from test_gpu_parity import TOL_LOGIT, TOL_PROB, TOL_VALUE

pytestmark = pytest.mark.gpu

KW = dict(logits=True, probs=True, value=True)
KEYS = ("logits", "probs", "value")
_fresh = {}            # (case, precision) -> the outputs of a fresh engine on the 32 rows


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


def _fresh_outputs(name, precision):
    """the request of the 32 rows on a fresh engine -> (outputs, fallbacks counted after it, rows 0 and 31 alone)"""
    from bokego_amd.engine import LeafEngine
    if (name, precision) not in _fresh:
        x = W.planes(name)
        eng = LeafEngine(*W.nets(name), max_batch=64, precision=precision)
        try:
            assert eng.precision == precision
            out = eng.eval(x, **KW)
            st = eng.stats()
            alone = {i: eng.eval(x[i:i + 1], **KW) for i in (0, 31)}
        finally:
            eng.close()
        _fresh[(name, precision)] = (out, st["f16_overflow_fallbacks"], alone)
    return _fresh[(name, precision)]


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", W.NAMES)
def test_case_vs_float64(name, precision):
    r = W.reference(name)
    out, fallbacks, alone = _fresh_outputs(name, precision)
    lg, pr, va = (out[k].astype(np.float64) for k in KEYS)
    d = W.delta(name, TOL_LOGIT)
    own = W.softmax64(out["logits"])
    fig = {"logits / delta": np.abs(lg - r.lg64).max() / d, "value / TOL_VALUE": np.abs(va - r.va64).max() / TOL_VALUE,
           "probs vs softmax64(own logits) / TOL_PROB": np.abs(pr - own).max() / TOL_PROB,
           "probs vs softmax64(lg64) / (delta / 2)": np.abs(pr - r.pr64).max() / (d / 2),
           "row sums / 1e-5": np.abs(pr.sum(1) - 1).max() / 1e-5}
    print(f"{name} {precision}: A {r.A:.4g} delta {d:.3g} fallbacks {fallbacks}; share of each bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    assert all(np.isfinite(out[k]).all() for k in KEYS)
    assert np.abs(lg - r.lg64).max() < d
    assert np.abs(va - r.va64).max() < TOL_VALUE
    assert (np.abs(va) <= 1).all()
    assert np.abs(pr - own).max() < TOL_PROB               # the softmax head on its own, underflowing probabilities included
    assert np.abs(pr - r.pr64).max() < d / 2               # softmax's Lipschitz bound: |dp_i| <= 2 p_i (1 - p_i) max|dlogit|
    assert np.abs(pr.sum(1) - 1).max() < 1e-5
    if name == "uniform_policy":
        assert np.array_equal(_bits(out["logits"]), np.full((32, 81), np.float32(0.25)).view(np.uint32))
        assert (_bits(out["probs"]) == _bits(out["probs"])[:, :1]).all()
        assert np.abs(pr - 1 / 81).max() < TOL_PROB
    # the fallback: none below the flag, exactly one above it -- and then the fp32 kernel's bits
    assert r.A < W.FLAG_AT / 2 or r.A > W.FLAG_AT * 2
    if precision == "f32" or r.A < W.FLAG_AT / 2:
        assert fallbacks == 0
    else:
        assert fallbacks == 1
        assert _same_bits(out, _fresh_outputs(name, "f32")[0])
    # rows 0 and 31 alone (B = 1: the cooperative form on the fp32 engine) have the bits they had inside the request
    for i, one in alone.items():
        for k in KEYS:
            assert np.array_equal(_bits(one[k]), _bits(out[k][i:i + 1])), (i, k)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["neg_gamma", "tiny_var_small_w", "huge_fold"])
def test_set_weights_on_a_live_engine(name, precision):
    """An engine that has served the golden nets takes the case's weights: the bits of an engine created with them, and the
    fallbacks of one (a net that does not fit fp16 is found when it arrives, not only at bk_engine_create)."""
    from bokego_amd.bkw import load_bkw
    from bokego_amd.engine import LeafEngine
    want, want_fallbacks, _ = _fresh_outputs(name, precision)
    x = W.planes(name)
    eng = LeafEngine(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw")),
                     max_batch=64, precision=precision)
    try:
        before = eng.eval(x, **KW)
        assert eng.stats()["f16_overflow_fallbacks"] == 0
        eng.set_weights(*W.nets(name))
        got = eng.eval(x, **KW)
        assert eng.stats()["f16_overflow_fallbacks"] == want_fallbacks
    finally:
        eng.close()
    assert not _same_bits(before, got)
    assert _same_bits(got, want)


def test_float_planes_beyond_fp16_are_redone_in_fp32():
    """The input side of the same promise, on the golden nets: a finite float plane of 65520 or more has no fp16 value (its hi
    half is Inf, its lo half -Inf), the matrix unit makes a NaN of it, and the epilogue's flag, a running fmaxf, drops that
    NaN while its ReLU hands on a 0.  The f16x2 kernel raises its flag for such a plane when it stages it, so the request is
    redone: one fallback, the fp32 kernel's bits, and float64's numbers within the bound every case above is held to."""
    from bokego_amd.bkw import load_bkw
    from bokego_amd.engine import LeafEngine
    pw, vw = load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw"))
    x = W.big_planes()
    out = {}
    for precision in ("f32", "f16x2"):
        eng = LeafEngine(pw, vw, max_batch=64, precision=precision)
        try:
            out[precision] = eng.eval(x, **KW)
            assert eng.stats()["f16_overflow_fallbacks"] == (precision == "f16x2")
        finally:
            eng.close()
    assert _same_bits(out["f16x2"], out["f32"])
    lg64, va64, _, _ = W.big_planes_reference()
    d = TOL_LOGIT * max(1.0, float(np.abs(lg64).max()) / 15.0)
    print(f"planes x 70000: |lg64|max {np.abs(lg64).max():.4g}, logits / delta {np.abs(out['f32']['logits'] - lg64).max() / d:.3f}, "
          f"value / TOL_VALUE {np.abs(out['f32']['value'] - va64).max() / TOL_VALUE:.3f}")
    assert all(np.isfinite(out["f32"][k]).all() for k in KEYS)
    assert np.abs(out["f32"]["logits"] - lg64).max() < d and np.abs(out["f32"]["value"] - va64).max() < TOL_VALUE


def test_a_net_that_does_not_fit_fp16_on_the_device_path():
    """bk_eval_device* of an f16x2 engine on huge_fold: the fp32 kernel's bits (no f16x2 launch, no gated redo), counted in
    f16_device_overflow."""
    import torch
    from bokego_amd.engine import LeafEngine
    want = _fresh_outputs("huge_fold", "f32")[0]
    eng = LeafEngine(*W.nets("huge_fold"), max_batch=64, precision="f16x2")
    try:
        got = eng.eval_device(torch.from_numpy(W.planes("huge_fold").copy()).cuda(), **KW)
        torch.cuda.synchronize()
        got = {k: got[k].cpu().numpy() for k in KEYS}
        st = eng.stats()
    finally:
        eng.close()
    assert st["f16_device_overflow"] == 1 and st["f16_overflow_fallbacks"] == 0
    assert _same_bits(got, want)

"""-m gpu: one NaN, +Inf or -Inf through every training entry point of libbktrain.so, against float64 torch.

The cases and their reference are tests/nonfinite_cases.py's (tests/test_nonfinite_cpu.py shows on the reference alone that
none of them is vacuous); the rule every element of every output is held to is nonfinite_cases.rule_violations, the
"Non-finite values" paragraph of include/bokego_train.h.  A test is one (precision, setup, operand, kind) and runs the
poison through every position of that operand; the clean call each one is compared with bit for bit is made once per
(precision, setup) and is itself held to test_gpu_train._bound_ok.

The gradients of BatchNorm + ReLU are handed y (and save_mean, save_invstd) of the float64 forward on the same poisoned
operands, rounded to float32: what the kernel under test computes does not depend on another kernel's answer.

Two places where the kernels have code of their own to land on the reference's set: a non-finite weight in
conv_dgrad, where torch's conv2d_input sums the taps on the board only (the plain forward-problem GEMM multiplies the zero
padding: 17 more NaN points per board), and gamma = +-Inf in the BatchNorm forward calls, where torch's CPU batch_norm
evaluates x * a + (beta - mean * a) and gives NaN where x and the mean have one sign.
"""
import math
import os

import numpy as np
import pytest
import torch

import nonfinite_cases as N
from bokego_amd import _trainlib as T
from bokego_amd import train
from conftest import GOLDEN
from test_gpu_train import _bound_ok

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U = 2.0 ** -23                          # test_gpu_train_bf16's unit: one fp32 addition of the matrix unit
R = 2.0 ** -8 + 2.0 ** -18              # ... and its bound of rounding both operands of a product to bf16


def _precisions(setup):
    return ("fp32", "bf16") if setup.op.startswith("conv_") else ("fp32",)     # BatchNorm has one form: fp32


def run(setup, o, hand, precision):
    """The _trainlib call of the setup on operands o (CPU float32) -> {output name: tensor on the GPU}."""
    op, B, cin, k = setup
    g = {n: v.to(DEV) for n, v in o.items()}
    h = {n: v.float().to(DEV) for n, v in hand.items()}
    if op == "conv_forward":
        return {"y": T.conv_forward(g["x"], g["w"], g["bias"], precision=precision)}
    if op == "conv_dgrad":
        return {"dx": T.conv_dgrad(g["dy"], g["w"], precision=precision)}
    if op == "conv_wgrad":
        dw, db = T.conv_wgrad(g["x"], g["dy"], (N.C, cin, k, k), precision=precision)
        return {"dw": dw, "db": db}
    if op == "bn_relu_train":
        rm, rv = g["running_mean"].clone(), g["running_var"].clone()
        nbt = torch.tensor(0, dtype=torch.int64, device=DEV)
        y, mean, invstd = T.bn_relu_train(g["x"], g["gamma"], g["beta"], rm, rv, nbt, N.MOMENTUM, N.EPS)
        return {"y": y, "save_mean": mean, "save_invstd": invstd, "running_mean": rm, "running_var": rv,
                "num_batches_tracked": nbt}
    if op == "bn_relu_eval":
        return {"y": T.bn_relu_eval(g["x"], g["gamma"], g["beta"], g["running_mean"], g["running_var"], N.EPS)}
    if op == "bn_relu_backward":
        out = T.bn_relu_backward(g["dy"], h["y"], g["x"], g["gamma"], h["save_mean"], h["save_invstd"])
    else:
        out = T.bn_relu_eval_backward(g["dy"], h["y"], g["x"], g["gamma"], g["running_mean"], g["running_var"], N.EPS)
    return dict(zip(("dx", "dgamma", "dbeta"), out))


_clean = {}


def clean_run(case, precision):
    """The kernel's outputs on the clean operands of the case, on the CPU; one call per (precision, setup)."""
    key = (precision, case.setup, case.where == "zero_weight")
    if key not in _clean:
        _, hand = N.clean_reference(case)
        _clean[key] = {n: v.cpu() for n, v in run(case.setup, N.clean(case), hand, precision).items()}
    return _clean[key]


def _clean_factors(setup, precision):
    """test_gpu_train's factor; for the bf16 forms test_gpu_train_bf16's, which adds the rounding of the operands"""
    if precision == "fp32":
        return {}
    K = setup.cin * setup.k * setup.k
    return {"y": R + (K + 1) * U, "dx": R + K * U, "dw": R + (16 * 81 + math.ceil(setup.B / 16)) * U}


@pytest.mark.parametrize("precision,setup", [(p, s) for s in N.setups() for p in _precisions(s)],
                         ids=lambda v: v if isinstance(v, str) else N.setup_id(v))
def test_the_clean_call_is_within_its_bound(precision, setup):
    case = N.cases(setup)[0]
    got, (ref, _), absref = clean_run(case, precision), N.clean_reference(case), N.abs_reference(setup, N.operands(setup))
    factors = _clean_factors(setup, precision)
    for name in N.OUTPUTS[setup.op]:
        if name == "num_batches_tracked":
            assert got[name].item() == 1
        else:
            assert got[name].isfinite().all(), name
            _bound_ok(got[name], ref[name], absref[name], factors.get(name, 2e-6))


def _groups():
    out = []
    for s in N.setups():
        seen = []
        for c in N.cases(s):
            if (c.operand, c.kind) not in seen:
                seen.append((c.operand, c.kind))
        out += [(p, s, operand, kind) for p in _precisions(s) for operand, kind in seen]
    return out


@pytest.mark.parametrize("precision,setup,operand,kind", _groups(),
                         ids=lambda v: v if isinstance(v, str) else N.setup_id(v))
def test_poison_goes_where_float64_sends_it(precision, setup, operand, kind):
    inf_may_be_nan = precision == "fp32" and setup.op.startswith("conv_")     # the compensated sums only
    bad = []
    for case in N.cases(setup):
        if (case.operand, case.kind) != (operand, kind):
            continue
        (ref, hand), (ref_clean, _) = N.case_reference(case), N.clean_reference(case)
        got, got_clean = run(setup, N.poisoned(case), hand, precision), clean_run(case, precision)
        for name in N.OUTPUTS[setup.op]:
            v = N.rule_violations(got[name], ref[name], got_clean[name], ref_clean[name],
                                  inf_may_be_nan and name != "db")            # db is a plain sum in double
            print(f"{N.case_id(case)} {name}: non-finite {int((~ref[name].double().isfinite()).sum())} of "
                  f"{ref[name].numel()}, violations {v}")
            if v:
                bad.append((N.case_id(case), name, v))
    assert not bad, bad


@pytest.mark.parametrize("precision", T.PRECISIONS)
@pytest.mark.parametrize("which", ["policy", "value"])
def test_one_training_step_with_a_nan_weight(which, precision):
    """One NaN in conv.9.weight: the loss is NaN, as float64's is, and the finite-mask of every parameter gradient and of
    every BatchNorm buffer after the step is float64's (test_nonfinite_cpu.py says what those masks are)."""
    sd, x, tp, tv = N.step_inputs(which)
    want_loss, want_grads, want_bufs = N.step_reference(which)
    cls = train.TrainablePolicyNet if which == "policy" else train.TrainableValueNet
    net = cls.from_state_dict(sd, device=DEV, precision=precision).train()
    out = net(x.to(DEV))
    loss = train.policy_loss(out, tp.to(DEV)) if which == "policy" else train.value_loss(out, tv.to(DEV))
    loss.backward()
    print(f"loss {loss.item()} (float64: {want_loss})")
    assert math.isnan(want_loss) and math.isnan(loss.item())
    grads = {n: p.grad.isfinite().cpu() for n, p in net.named_parameters()}
    assert set(grads) == set(want_grads)
    bad = [n for n in grads if not torch.equal(grads[n], want_grads[n])]
    assert not bad, bad
    bufs = {n: b.isfinite().cpu() for n, b in net.named_buffers() if b.dtype.is_floating_point}
    assert set(bufs) == set(want_bufs)
    bad = [n for n in bufs if not torch.equal(bufs[n], want_bufs[n])]
    assert not bad, bad


# ---- the engine refuses what the kernels above would pass on ----------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_a_live_engine_refuses_poisoned_weights_and_serves_the_old_ones():
    """bk_engine_set_weights with one NaN or Inf anywhere: BK_ERR_ARG naming the net and the tensor, and every output bit of
    the next requests as before (the pattern of test_gpu_hooks.test_new_weights_arrive_all_or_not_at_all)."""
    from bokego_amd.bkw import load_bkw
    from bokego_amd.engine import LeafEngine
    pw, vw = load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw"))
    x = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"][:300].astype(np.uint8)
    eng = LeafEngine(pw, vw, max_batch=512)
    try:
        kw = dict(logits=True, probs=True, value=True)
        before = [eng.eval(x[:B], **kw) for B in (5, 300)]
        for net, name, at, value in (("policy", "conv.6.weight", 12345, np.nan), ("policy", "conv.21.bias", -1, np.inf),
                                     ("value", "conv.0.weight", 0, -np.inf), ("value", "lin1.weight", -1, np.nan),
                                     ("value", "conv.10.running_var", 7, -1.0)):
            sd = dict(pw if net == "policy" else vw)
            a = np.array(sd[name], np.float32)
            a.reshape(-1)[at] = value
            sd[name] = a
            with pytest.raises(ValueError, match=f"BK_ERR_ARG: weights are not finite: {net} {name}$".replace(".", r"\.")):
                eng.set_weights(**{f"{net}_sd": sd})
            after = [eng.eval(x[:B], **kw) for B in (5, 300)]
            assert all(_same(a_, b_) for a_, b_ in zip(before, after)), (net, name)
        with pytest.raises(RuntimeError, match="BK_ERR_ARG: weights are not finite: policy conv.6.weight"):
            bad = dict(pw)
            bad["conv.6.weight"] = np.full_like(np.array(pw["conv.6.weight"], np.float32), np.nan)
            LeafEngine(bad, None, max_batch=16)
    finally:
        eng.close()


def test_a_net_with_a_nan_is_refused_by_its_engine():
    """HipPolicyNet makes its engine at the first evaluation: that is where a state_dict with a NaN is refused; a live net
    refuses it in load_state_dict, keeps its weights and answers as before."""
    from bokego_amd import nnet
    from bokego_amd.bkw import load_bkw
    sd = dict(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    a = np.array(sd["conv.9.weight"], np.float32)
    a[5, 7, 1, 1] = np.nan
    x = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"][:5].astype(np.float32)
    with pytest.raises(RuntimeError, match=r"BK_ERR_ARG: weights are not finite: policy conv\.9\.weight"):
        nnet.HipPolicyNet({**sd, "conv.9.weight": a})(x)
    net = nnet.HipPolicyNet(sd)
    before = torch.as_tensor(net(x)).clone()
    with pytest.raises(ValueError, match=r"weights are not finite: policy conv\.9\.weight"):
        net.load_state_dict({**sd, "conv.9.weight": a})
    assert torch.equal(torch.as_tensor(net(x)), before)
    assert np.isfinite(net._sd["conv.9.weight"]).all()
    net._drop_engine()

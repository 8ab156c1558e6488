"""One NaN, +Inf or -Inf in one operand of one training kernel, with what float64 torch makes of it.

Shared by test_nonfinite_cpu.py (the reference alone: every case does something, and the affected sets have the shapes
the kernels' contract quotes) and test_gpu_nonfinite.py (the kernels of libbktrain.so against the same reference), so
that the GPU comparison can never pass on an empty set.  Everything is built in code; there is no fixture.

A case is (setup, operand to poison, flat index into it, kind).  A setup is (operation, B, cin, k); its clean operands are
seeded normals of moderate size with no exact zero anywhere, so that Inf * 0 arises only where an operation itself brings
a zero in: the zero padding of a convolution and the masked tails of the kernels.  One extra named case per convolution
puts an exact zero weight against an Inf input.  No large finite values: fp32 overflow where float64 stays finite is
another subject.

The reference of each operation is plain float64 torch on the CPU: F.conv2d, torch.nn.grad.conv2d_weight / conv2d_input,
F.batch_norm + torch.relu with autograd -- what test_gpu_train.py uses for finite inputs.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

NAN, INF = float("nan"), float("inf")
KINDS = {"nan": NAN, "+inf": INF, "-inf": -INF}
EPS, MOMENTUM = 1e-5, 0.1
C = 128                                   # output channels of every convolution, channels of every BatchNorm

Setup = collections.namedtuple("Setup", "op B cin k")
Case = collections.namedtuple("Case", "setup operand index kind where")

CONV_SHAPES = ((27, 5), (128, 3))
BATCHES = (1, 17)                          # 17: two slices of BKT_WGRAD_CHUNK = 16 boards with one board in the second, and
                                           # the 64-column tile boundary inside board 0 (1377 columns = 21 * 64 + 33)
OPS = ("conv_forward", "conv_dgrad", "conv_wgrad", "bn_relu_train", "bn_relu_backward", "bn_relu_eval",
       "bn_relu_eval_backward")
# what each operation hands back, in the order of the _trainlib call
OUTPUTS = {"conv_forward": ("y",), "conv_dgrad": ("dx",), "conv_wgrad": ("dw", "db"),
           "bn_relu_train": ("y", "save_mean", "save_invstd", "running_mean", "running_var", "num_batches_tracked"),
           "bn_relu_backward": ("dx", "dgamma", "dbeta"), "bn_relu_eval": ("y",),
           "bn_relu_eval_backward": ("dx", "dgamma", "dbeta")}


def setups():
    out = []
    for B in BATCHES:
        for cin, k in CONV_SHAPES:
            out += [Setup("conv_forward", B, cin, k), Setup("conv_wgrad", B, cin, k)]
        out.append(Setup("conv_dgrad", B, C, 3))
        out += [Setup(op, B, C, 0) for op in OPS if op.startswith("bn_")]
    return out


def _normal(shape, seed, scale=1.0, shift=0.0, positive=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    a = (a.abs() if positive else a) * scale + shift
    a = a.float()
    assert (a != 0).all()                  # no exact zero: Inf * 0 comes from padding and masked tails only
    return a


@functools.lru_cache(maxsize=None)
def operands(setup):
    """The clean operands of a setup, float32 on the CPU, by name.  Shared: never written to."""
    op, B, cin, k = setup
    s = 7919 * B + 31 * cin + k
    if op.startswith("conv_"):
        o = {"x": _normal((B, cin, 9, 9), s), "w": _normal((C, cin, k, k), s + 1, 0.1),
             "bias": _normal((C,), s + 2), "dy": _normal((B, C, 9, 9), s + 3)}
        keep = {"conv_forward": ("x", "w", "bias"), "conv_dgrad": ("dy", "w"), "conv_wgrad": ("x", "dy")}[op]
        return {n: o[n] for n in keep}
    o = {"x": _normal((B, C, 9, 9), s + 4, 3.0, 0.5), "gamma": _normal((C,), s + 5, 0.5, 0.5, positive=True),
         "beta": _normal((C,), s + 6, 0.2), "running_mean": _normal((C,), s + 7, 0.1),
         "running_var": _normal((C,), s + 8, 1.0, 0.5, positive=True), "dy": _normal((B, C, 9, 9), s + 9)}
    # where the poison goes, the clean ReLU is open at "first", "last" and "centre" (x = 4: y > 0 whatever gamma > 0 and beta
    # are) and shut at "corner" (x = -4: y = 0), so that both sides of the mask are met by construction
    for where, idx in _positions("x", (B, C, 9, 9)).items():
        o["x"].view(-1)[idx] = -4.0 if where == "corner" else 4.0
    keep = {"bn_relu_train": ("x", "gamma", "beta", "running_mean", "running_var"),
            "bn_relu_backward": ("x", "gamma", "beta", "dy"),
            "bn_relu_eval": ("x", "gamma", "beta", "running_mean", "running_var"),
            "bn_relu_eval_backward": ("x", "gamma", "beta", "running_mean", "running_var", "dy")}[op]
    return {n: o[n] for n in keep}


def _positions(name, shape):
    """{label: flat index}: where the poison goes in an operand of that name and shape."""
    n = math.prod(shape)
    if len(shape) == 4 and shape[2:] == (9, 9):            # activations [B, channels, 9, 9]
        B, ch = shape[0], shape[1]
        return {"first": 0,
                "last": n - 1,                             # last board, last channel, point 80: tail tile, tail slice
                "corner": (0 * ch + min(1, ch - 1)) * 81 + 8,                     # board 0, channel 1, point (0, 8)
                "centre": ((B // 2) * ch + ch // 2) * 81 + 40}                    # a middle board and channel, point (4, 4)
    # weights [128, cin, k, k]: (m=0, ci=0, tap 0) and (m=127, ci=cin-1, last tap), the last K row of a partial stage;
    # per-channel vectors [128]: channel 0 and channel 127
    return {"first": 0, "last": n - 1}


def cases(setup):
    out = []
    for name, t in operands(setup).items():
        for where, idx in _positions(name, tuple(t.shape)).items():
            for kind in KINDS:
                out.append(Case(setup, name, idx, kind, where))
        if name == "running_var":          # the square root of a negative number
            for where, idx in _positions(name, tuple(t.shape)).items():
                out.append(Case(setup, name, idx, "-1", where))
    if setup.op in ("conv_forward", "conv_dgrad"):
        out.append(Case(setup, "x" if setup.op == "conv_forward" else "dy", None, "+inf", "zero_weight"))
    return out


def case_id(c):
    return f"{c.operand}-{c.where}-{c.kind}"


def setup_id(s):
    return f"{s.op}-B{s.B}" + (f"-cin{s.cin}-k{s.k}" if s.op.startswith("conv_") else "")


# the named case: +Inf at the centre of board 0, channel 0, against w[ZERO_M, 0, centre tap] == 0 exactly.  Output channel
# ZERO_M is NaN at that point (Inf * 0) and the other channels are +-Inf there.
ZERO_M = 77


@functools.lru_cache(maxsize=None)
def _zero_weight_operands(setup):
    o = dict(operands(setup))
    w, k = o["w"].clone(), setup.k
    if setup.op == "conv_forward":
        w[ZERO_M, 0, k // 2, k // 2] = 0.0                 # y[0, m, 4, 4] takes x[0, 0, 4, 4] * w[m, 0, centre]
    else:
        w[0, ZERO_M, 1, 1] = 0.0                           # dx[0, ci, 4, 4] takes dy[0, 0, 4, 4] * w[0, ci, centre]
    o["w"] = w
    return o


def clean(case):
    """The operands the case starts from: the setup's, or for the named case the setup's with its one zero weight."""
    return _zero_weight_operands(case.setup) if case.where == "zero_weight" else operands(case.setup)


def poisoned(case):
    """The operands of the case: the clean ones with one element of one operand replaced (a copy of that operand)."""
    o = dict(clean(case))
    if case.where == "zero_weight":
        a = o[case.operand].clone()
        a[0, 0, 4, 4] = INF
        o[case.operand] = a
        return o
    a = o[case.operand].clone()
    a.view(-1)[case.index] = KINDS[case.kind] if case.kind in KINDS else float(case.kind)
    o[case.operand] = a
    return o


def _bn_outputs(setup, d, train):
    x, gamma, beta = d["x"].requires_grad_(True), d["gamma"].requires_grad_(True), d["beta"].requires_grad_(True)
    if train and "running_mean" not in d:  # the backward setups have no running buffers
        rm = rv = None
    else:
        rm, rv = d["running_mean"].clone(), d["running_var"].clone()
    y = torch.relu(F.batch_norm(x, rm, rv, gamma, beta, training=train, momentum=MOMENTUM, eps=EPS))
    return x, gamma, beta, rm, rv, y


def reference(setup, o):
    """float64 torch -> (outputs by name, what the GPU call is handed from the forward: y, and for the train-mode gradient
    save_mean and save_invstd).  The gradients are autograd's through batch_norm and relu."""
    op, B, cin, k = setup
    d = {n: v.double() for n, v in o.items()}
    if op == "conv_forward":
        return {"y": F.conv2d(d["x"], d["w"], d["bias"], padding=k // 2)}, {}
    if op == "conv_dgrad":
        return {"dx": torch.nn.grad.conv2d_input(d["dy"].shape, d["w"], d["dy"], padding=1)}, {}
    if op == "conv_wgrad":
        return {"dw": torch.nn.grad.conv2d_weight(d["x"], (C, cin, k, k), d["dy"], padding=k // 2),
                "db": d["dy"].sum((0, 2, 3))}, {}
    train = op in ("bn_relu_train", "bn_relu_backward")
    x, gamma, beta, rm, rv, y = _bn_outputs(setup, d, train)
    hand = {"y": y.detach()}
    if train:
        xd = x.detach()
        mean = xd.mean((0, 2, 3))
        hand["save_mean"] = mean
        hand["save_invstd"] = 1.0 / torch.sqrt(xd.var((0, 2, 3), unbiased=False) + EPS)
    if op == "bn_relu_train":
        return {"y": y.detach(), "save_mean": hand["save_mean"], "save_invstd": hand["save_invstd"], "running_mean": rm,
                "running_var": rv, "num_batches_tracked": torch.tensor(1, dtype=torch.int64)}, hand
    if op == "bn_relu_eval":
        return {"y": y.detach()}, hand
    y.backward(d["dy"])
    return {"dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad}, hand


def abs_reference(setup, o):
    """sum |a * b| of every output of the clean call: the same operation on the operands' absolute values, written out
    for BatchNorm term by term.  The scale of test_gpu_train._bound_ok's elementwise error bound."""
    op, B, cin, k = setup
    d = {n: v.double() for n, v in o.items()}
    if op.startswith("conv_"):
        out, _ = reference(setup, {n: v.abs() for n, v in o.items()})
        return out
    bc = lambda v: v.reshape(1, C, 1, 1)
    x = d["x"]
    n = B * 81
    train = op in ("bn_relu_train", "bn_relu_backward")
    if train:
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    else:
        mean, var = d["running_mean"], d["running_var"]
    invstd = 1.0 / torch.sqrt(var + EPS)
    ax = (x.abs() + bc(mean.abs())) * bc(invstd)           # |x| * invstd + |mean| * invstd: the terms of xhat
    y_abs = ax * bc(d["gamma"].abs()) + bc(d["beta"].abs())
    if op == "bn_relu_eval":
        return {"y": y_abs}
    if op == "bn_relu_train":
        m1, m2 = x.abs().mean((0, 2, 3)), (x * x).mean((0, 2, 3))
        return {"y": y_abs, "save_mean": m1, "save_invstd": invstd,
                "running_mean": (1 - MOMENTUM) * d["running_mean"].abs() + MOMENTUM * m1,
                "running_var": (1 - MOMENTUM) * d["running_var"].abs() + MOMENTUM * (m2 + mean * mean) * n / (n - 1.0),
                "num_batches_tracked": torch.tensor(0, dtype=torch.int64)}
    dz = d["dy"].abs()                                     # every |dy|: an upper bound of |dz|
    s_dz, s_dzx = dz.sum((0, 2, 3)), (dz * ax).sum((0, 2, 3))
    scale = bc(d["gamma"].abs() * invstd)
    if op == "bn_relu_eval_backward":
        return {"dx": dz * scale, "dgamma": s_dzx, "dbeta": s_dz}
    return {"dx": scale * (dz + bc(s_dz) / n + ax * bc(s_dzx) / n), "dgamma": s_dzx, "dbeta": s_dz}


@functools.lru_cache(maxsize=None)
def _clean_reference(setup, zero_weight):
    return reference(setup, _zero_weight_operands(setup) if zero_weight else operands(setup))


def clean_reference(case):
    return _clean_reference(case.setup, case.where == "zero_weight")


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return reference(case.setup, poisoned(case))


def same_bits(a, b):
    """elementwise: the same value bit for bit (any NaN equals any NaN, -0 differs from +0)"""
    if not a.dtype.is_floating_point:
        return a == b
    bits = {torch.float64: torch.int64, torch.float32: torch.int32}[a.dtype]
    return (a.contiguous().view(bits) == b.contiguous().view(bits)) | (a.isnan() & b.isnan())


# ---- the rule ----------------------------------------------------------------------------------------------------------
CHANGED_TOL = 2e-5


def rule_violations(got, ref, got_clean, ref_clean, inf_may_be_nan):
    """The non-finite contract of include/bokego_train.h, applied to every element of one output.  got / got_clean: the
    kernel's float32 (or int64) result on the poisoned / the clean operands; ref / ref_clean: float64 torch on the same.
    -> {what is violated: number of elements}, empty when the output keeps the contract.

      finite    isfinite(got) == isfinite(ref)
      nan       ref is NaN: got is NaN
      inf       ref is +-Inf: got is the same Inf -- or, with inf_may_be_nan (the fp32 convolutions' compensated sums:
                (t - acc) - y is inf - inf once a running sum is Inf), NaN
      bits      ref is finite and has the bits of ref_clean -- the element does not depend on the poison: got has the
                bits of got_clean.  The kernels' summation order does not depend on values, so there is no tolerance.
      changed   ref is finite but not ref_clean's: the poison reached the element and left it finite (ReLU of -Inf is 0, a
                NaN output lets its gradient term into a sum, a variance of +Inf is a scale of 0).  Such an element has no
                clean twin, so it is held to float32's precision: |got - ref| <= 2e-5 * (1 + |ref|), the absolute figure
                test_gpu_train.py holds BatchNorm outputs of this size to.
    """
    if not ref.dtype.is_floating_point:
        n = int((got.cpu() != ref).sum())
        return {"integer": n} if n else {}
    g, gc = got.detach().cpu(), got_clean.detach().cpu()
    g64 = g.double()
    fin = ref.isfinite()
    unchanged = fin & same_bits(ref, ref_clean)
    changed = fin & ~unchanged
    same_inf = g64 == ref
    if inf_may_be_nan:
        same_inf = same_inf | g64.isnan()
    bad = {"finite": g64.isfinite() != fin,
           "nan": ref.isnan() & ~g64.isnan(),
           "inf": ref.isinf() & ~same_inf,
           "bits": unchanged & ~same_bits(g, gc),
           "changed": changed & ~((g64 - ref).abs() <= CHANGED_TOL * (1 + ref.abs()))}
    return {k: int(v.sum()) for k, v in bad.items() if v.any()}


# ---- one training step with one NaN weight -------------------------------------------------------------------------------
STEP_BATCH = 17
STEP_POISON = ("conv.9.weight", (5, 7, 1, 1))            # one NaN in the fourth trunk convolution


def step_inputs(which):
    """-> (state_dict with the one NaN, planes float32 [17,27,9,9], policy targets [17,81], value targets [17]) of the net
    `which` ("policy" or "value"), from the golden weights and features."""
    import os

    import numpy as np

    from bokego_amd import train
    from conftest import GOLDEN
    from test_gpu_train import _targets

    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw" if which == "policy" else "value_synth.bkw"))
    sd = {k: v.clone() for k, v in sd.items()}
    name, at = STEP_POISON
    assert sd[name][at].isfinite()
    sd[name][at] = NAN
    feats = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"][:STEP_BATCH].astype(np.float32)
    tp, tv = _targets(STEP_BATCH, 5)
    return sd, torch.from_numpy(feats), tp, tv


@functools.lru_cache(maxsize=None)
def step_reference(which):
    """The step in float64 (test_gpu_train.Ref64) -> (loss, {parameter: finite-mask of its gradient}, {BatchNorm buffer:
    finite-mask after the step})."""
    from bokego_amd import train
    from test_gpu_train import Ref64

    sd, x, tp, tv = step_inputs(which)
    ref = Ref64(sd, which == "value")
    out = ref(x)
    loss = train.policy_loss(out, tp.double()) if which == "policy" else train.value_loss(out, tv.double())
    loss.backward()
    return (loss.item(), {n: p.grad.isfinite() for n, p in ref.p.items()},
            {n: b.isfinite() for n, b in ref.buf.items() if b.dtype.is_floating_point})

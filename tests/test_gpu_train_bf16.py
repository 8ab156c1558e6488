"""-m gpu: the bf16 mixed-precision mode of the training kernels (precision="bf16") on the MI355X.

The contract (include/bokego_train.h): fp32 tensors; each GEMM operand element rounded once to bf16, round to nearest
even; exact products, fp32 accumulation; bias added unrounded; db from the unrounded dy.  r(t) = t.bfloat16().float()
is that rounding (torch's cast is RNE).  The yardsticks are float64 torch on the CPU and, for a whole training step,
the *ideal* mixed-precision model: the float64 network with the two operands of each of a trunk convolution's three
GEMMs rounded to bf16 and everything else in float64.  It is restated here with torch ops and shares no code with the
kernels."""
import copy
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bokego_amd import _trainlib as T
from bokego_amd import nnet, reinforce, selfplay, train
from bokego_amd.bkw import load_bkw
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CONV = (0, 3, 6, 9, 12, 15, 18)
DEV = torch.device("cuda", 0)
U = 2.0 ** -23                     # one fp32 addition, whether the MFMA's internal sum rounds or truncates


def r(t):
    return t.bfloat16().to(t.dtype)


def _seeded(shape, seed, zero_frac=0.2):
    """normal values of both signs with a share of exact zeros"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    a[torch.rand(shape, generator=g) < zero_frac] = 0
    return a.float()


def _bound_ok(got, ref, absref, factor, what=""):
    """|got - ref| <= factor * sum|a*b| elementwise (absref: the same operation on |a| and |b| in float64)"""
    d = (got.double().cpu() - ref).abs()
    lim = factor * absref + 1e-30
    worst = (d / lim).max().item()
    print(f"{what}: error {worst:.3g} x the bound (factor {factor:.3g})")
    assert worst <= 1.0, f"{what}: error {worst:.3g} x the bound"


# ---- the convolutions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 37, 256])
@pytest.mark.parametrize("cin,k", [(27, 5), (128, 3)])
def test_bf16_conv_kernels(B, cin, k):
    seed = 1000 * B + k
    x, w, b = _seeded((B, cin, 9, 9), seed), _seeded((128, cin, k, k), seed + 1) * 0.1, _seeded((128,), seed + 2)
    dy = _seeded((B, 128, 9, 9), seed + 3)
    pad = k // 2
    gx, gw, gb, gdy = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    grx, grw, grdy = r(x).to(DEV), r(w).to(DEV), r(dy).to(DEV)
    assert not torch.equal(r(x), x) and not torch.equal(r(w), w) and not torch.equal(r(dy), dy)

    # 3. rounding is where the contract says, exactly: rounding the operands beforehand changes no bit
    y = T.conv_forward(gx, gw, gb, precision="bf16")
    y_r = T.conv_forward(grx, grw, gb, precision="bf16")
    assert torch.equal(y, y_r)
    y32 = T.conv_forward(gx, gw, gb, precision="fp32")
    assert not torch.equal(y, y32)
    dw, db = T.conv_wgrad(gx, gdy, w.shape, precision="bf16")
    dw_r, _ = T.conv_wgrad(grx, grdy, w.shape, precision="bf16")
    assert torch.equal(dw, dw_r)
    if cin == 128:
        dx = T.conv_dgrad(gdy, gw, precision="bf16")
        dx_r = T.conv_dgrad(grdy, grw, precision="bf16")
        assert torch.equal(dx, dx_r)

    # 5. the same bits again, and "fp32" is the call without the keyword
    assert torch.equal(y, T.conv_forward(gx, gw, gb, precision="bf16"))
    dw2, db2 = T.conv_wgrad(gx, gdy, w.shape, precision="bf16")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.equal(y32, T.conv_forward(gx, gw, gb))
    dw32, db32 = T.conv_wgrad(gx, gdy, w.shape, precision="fp32")
    dw32b, db32b = T.conv_wgrad(gx, gdy, w.shape)
    assert torch.equal(dw32, dw32b) and torch.equal(db32, db32b)
    if cin == 128:
        assert torch.equal(dx, T.conv_dgrad(gdy, gw, precision="bf16"))
        assert torch.equal(T.conv_dgrad(gdy, gw, precision="fp32"), T.conv_dgrad(gdy, gw))

    # 4. accumulation is at least fp32: on the rounded operands only the summation errs
    xd, wd, bd, dyd = r(x).double(), r(w).double(), b.double(), r(dy).double()
    n_f, n_d, n_w = cin * k * k + 1, cin * k * k, 16 * 81 + math.ceil(B / 16)
    ref_y, abs_y = F.conv2d(xd, wd, bd, padding=pad), F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=pad)
    _bound_ok(y, ref_y, abs_y, n_f * U, "forward, rounded operands")
    ref_dw = torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, padding=pad)
    abs_dw = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), padding=pad)
    _bound_ok(dw, ref_dw, abs_dw, n_w * U, "weight gradient, rounded operands")
    _bound_ok(db, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)), 2e-6, "bias gradient (unrounded dy)")
    if cin == 128:
        _bound_ok(dx, torch.nn.grad.conv2d_input(xd.shape, wd, dyd, padding=pad),
                  torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), padding=pad), n_d * U,
                  "input gradient, rounded operands")

    # 3 and 4 together, on the unrounded inputs against the unrounded float64 reference
    R = 2.0 ** -8 + 2.0 ** -18
    xd, wd, dyd = x.double(), w.double(), dy.double()
    _bound_ok(y, F.conv2d(xd, wd, bd, padding=pad), F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=pad), R + n_f * U,
              "forward")
    _bound_ok(dw, torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, padding=pad),
              torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), padding=pad), R + n_w * U, "weight gradient")
    if cin == 128:
        _bound_ok(dx, torch.nn.grad.conv2d_input(xd.shape, wd, dyd, padding=pad),
                  torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), padding=pad), R + n_d * U, "input gradient")


def test_bf16_conv_refuses_what_it_does_not_support():
    x = torch.zeros((2, 27, 9, 9), device=DEV)
    with pytest.raises(ValueError):
        T.conv_forward(x, torch.zeros((128, 27, 4, 4), device=DEV), precision="bf16")
    with pytest.raises(ValueError):
        T.conv_dgrad(torch.zeros((2, 128, 9, 9), device=DEV), torch.zeros((128, 27, 5, 5), device=DEV),
                     precision="bf16")
    with pytest.raises(ValueError):
        T.conv_forward(x.cpu(), torch.zeros((128, 27, 5, 5)), precision="bf16")
    with pytest.raises(ValueError):
        T.conv_wgrad(x, torch.zeros((3, 128, 9, 9), device=DEV), (128, 27, 5, 5), precision="bf16")
    with pytest.raises(ValueError):
        T.conv_forward(x, torch.zeros((128, 27, 5, 5), device=DEV), precision="tf32")
    lib = T.load()
    assert lib.bkt_conv_packed_elems_bf16(27, 4) == 0 and lib.bkt_conv_packed_elems_bf16(0, 3) == 0
    assert lib.bkt_conv_packed_elems_bf16(27, 5) >= 128 * 27 * 25
    assert lib.bkt_conv_wgrad_workspace_bf16(0, 128, 3) == 0 and lib.bkt_conv_wgrad_workspace_bf16(2, 128, 7) == 0


# ---- the float64 models, from the state_dict with torch ops --------------------------------------------------------------
class _Bf16Conv(torch.autograd.Function):
    """The ideal mixed-precision convolution: each of the three GEMMs on operands rounded to bf16, all else float64."""

    @staticmethod
    def forward(ctx, x, w, b, pad):
        ctx.save_for_backward(x, w)
        ctx.pad = pad
        return F.conv2d(r(x), r(w), b, padding=pad)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = torch.nn.grad.conv2d_input(x.shape, r(w), r(dy), padding=ctx.pad)
        dw = torch.nn.grad.conv2d_weight(r(x), w.shape, r(dy), padding=ctx.pad)
        return dx, dw, dy.sum((0, 2, 3)), None


class Ref64:
    """The float64 network; ideal=True puts _Bf16Conv in place of the trunk convolutions."""

    def __init__(self, sd, value, ideal=False):
        self.value, self.ideal = value, ideal
        self.p, self.buf = {}, {}
        for k, v in sd.items():
            t = v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu().clone()
            if "running_" in k or k.endswith("num_batches_tracked"):
                self.buf[k] = t.clone()
            else:
                self.p[k] = t.clone().requires_grad_(True)

    def _bn(self, h, pre):
        self.buf[pre + ".num_batches_tracked"] += 1    # what nn.BatchNorm2d.forward does around F.batch_norm
        return F.batch_norm(h, self.buf[pre + ".running_mean"], self.buf[pre + ".running_var"], self.p[pre + ".weight"],
                            self.p[pre + ".bias"], training=True, momentum=0.1, eps=1e-5)

    def __call__(self, x):
        h = x.double()
        for l, c in enumerate(CONV):
            w, b, pad = self.p[f"conv.{c}.weight"], self.p[f"conv.{c}.bias"], 2 if l == 0 else 1
            h = _Bf16Conv.apply(h, w, b, pad) if self.ideal else F.conv2d(h, w, b, padding=pad)
            h = torch.relu(self._bn(h, f"conv.{c + 1}"))
        z = F.conv2d(h, self.p["conv.21.weight"]) + self.p["conv.21.bias"]
        if not self.value:
            return z.reshape(-1, 81)
        h = torch.relu(self._bn(z, "bn")).reshape(-1, 81)
        h = torch.relu(self._bn(F.linear(h, self.p["lin1.weight"], self.p["lin1.bias"]), "lin_bn"))
        return torch.tanh(F.linear(h, self.p["lin2.weight"], self.p["lin2.bias"]))


@pytest.fixture(scope="module")
def golden():
    feats = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"]
    return (feats, train.load_weights(os.path.join(GOLDEN, "policy_19.bkw")),
            train.load_weights(os.path.join(GOLDEN, "value_synth.bkw")))


def _targets(n, seed):
    rng = np.random.default_rng(seed)
    pol = rng.random((n, 81)).astype(np.float32) ** 4
    pol /= pol.sum(1, keepdims=True)
    val = rng.choice([-1.0, 1.0], n).astype(np.float32)
    return torch.from_numpy(pol), torch.from_numpy(val)


def _zero_by_bn(name):
    """biases followed by a train-mode BatchNorm: their gradient is zero in exact arithmetic"""
    return name in {f"conv.{c}.bias" for c in CONV} or name == "lin1.bias"


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("which", ["policy", "value"])
def test_one_bf16_training_step_against_the_ideal_model(golden, which):
    """e_gpu(p) <= 2 e_ideal(p) + 1e-4 for every parameter's gradient, the output and the running statistics, both
    errors relative to the float64 model.  Measured on the MI355X (worst e_gpu / e_ideal over the conv weights and
    BatchNorm parameters): see DESIGN 14."""
    feats, psd, vsd = golden
    sd = psd if which == "policy" else vsd
    cls = train.TrainablePolicyNet if which == "policy" else train.TrainableValueNet
    x = torch.from_numpy(feats[:256].astype(np.float32))
    tp, tv = _targets(256, 5)

    net = cls.from_state_dict(sd, device=DEV, precision="bf16").train()
    assert net.precision == "bf16"
    ref, ideal = Ref64(net.state_dict(), which == "value"), Ref64(net.state_dict(), which == "value", ideal=True)
    out = net(x.to(DEV))
    loss = train.policy_loss(out, tp.to(DEV)) if which == "policy" else train.value_loss(out, tv.to(DEV))
    loss.backward()
    outs = {}
    for name, m in (("ref", ref), ("ideal", ideal)):
        o = m(x)
        l = train.policy_loss(o, tp.double()) if which == "policy" else train.value_loss(o, tv.double())
        l.backward()
        outs[name] = o.detach()

    e_ideal, e_gpu = _rel(outs["ideal"], outs["ref"]), _rel(out.detach().double().cpu(), outs["ref"])
    print(f"{which} output: e_gpu {e_gpu:.3e} e_ideal {e_ideal:.3e}")
    assert e_gpu <= 2 * e_ideal + 1e-4
    grads = {n: p.grad.double().cpu() for n, p in net.named_parameters()}
    assert set(grads) == set(ref.p)
    bad = []
    for n, g in grads.items():
        want, mid = ref.p[n].grad, ideal.p[n].grad
        if _zero_by_bn(n):
            lim = 1e-6 * grads[n.replace(".bias", ".weight")].norm()
            print(f"{which} {n}: norm {g.norm().item():.3e} limit {lim.item():.3e}")
            if not (g.norm() <= lim and want.norm() <= lim):
                bad.append((n, g.norm().item(), lim.item()))
        else:
            e_ideal, e_gpu = _rel(mid, want), _rel(g, want)
            print(f"{which} {n}: e_gpu {e_gpu:.3e} e_ideal {e_ideal:.3e} ratio {e_gpu / max(e_ideal, 1e-300):.3f}")
            if e_gpu > 2 * e_ideal + 1e-4:
                bad.append((n, e_gpu, e_ideal))
    assert not bad, bad
    bufs = dict(net.named_buffers())
    for k, want in ref.buf.items():
        got = bufs[k].cpu()
        if k.endswith("num_batches_tracked"):
            assert got.item() == want.item() == ideal.buf[k].item() == 1, k
        else:
            e_ideal, e_gpu = _rel(ideal.buf[k], want), _rel(got.double(), want)
            print(f"{which} {k}: e_gpu {e_gpu:.3e} e_ideal {e_ideal:.3e}")
            assert e_gpu <= 2 * e_ideal + 1e-4, k


def _step(nets, opts, x, tp, tv):
    losses = []
    for n, net in nets.items():
        out = net(x)
        loss = train.policy_loss(out, tp) if n == "policy" else train.value_loss(out, tv)
        opts[n].zero_grad(set_to_none=True)
        loss.backward()
        opts[n].step()
        losses.append(loss.detach().clone())
    return losses


def _snapshot(nets, opts):
    return ({n: {k: v.detach().clone() for k, v in net.state_dict().items()} for n, net in nets.items()},
            {n: copy.deepcopy(o.state_dict()) for n, o in opts.items()})


def _bf16_nets(psd, vsd):
    return {"policy": train.TrainablePolicyNet.from_state_dict(psd, device=DEV, precision="bf16").train(),
            "value": train.TrainableValueNet.from_state_dict(vsd, device=DEV, precision="bf16").train()}


def test_bf16_steps_are_bit_deterministic(golden):
    feats, psd, vsd = golden
    x = torch.from_numpy(feats[:256]).to(DEV)
    tp, tv = (t.to(DEV) for t in _targets(256, 6))
    nets = _bf16_nets(psd, vsd)
    opts = {n: torch.optim.Adam(net.parameters(), lr=1e-3) for n, net in nets.items()}
    _step(nets, opts, x, tp, tv)                       # Adam has moments from here on
    sd0, os0 = _snapshot(nets, opts)
    l1 = _step(nets, opts, x, tp, tv)
    sd1, os1 = _snapshot(nets, opts)
    for n in nets:
        nets[n].load_state_dict(sd0[n])
        opts[n].load_state_dict(os0[n])
    l2 = _step(nets, opts, x, tp, tv)
    sd2, os2 = _snapshot(nets, opts)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    for n in nets:
        assert all(torch.equal(sd1[n][k], sd2[n][k]) for k in sd1[n])
        st1, st2 = os1[n]["state"], os2[n]["state"]
        assert st1.keys() == st2.keys()
        for i in st1:
            assert all(torch.equal(st1[i][k], st2[i][k]) for k in st1[i])
    assert not torch.equal(sd0["policy"]["conv.3.weight"], sd1["policy"]["conv.3.weight"])
    # precision is a plain attribute of a live net: the same step in fp32 mode gives other bits
    for n in nets:
        nets[n].load_state_dict(sd0[n])
        opts[n].load_state_dict(os0[n])
        nets[n].precision = "fp32"
    l3 = _step(nets, opts, x, tp, tv)
    assert not any(torch.equal(a, b) for a, b in zip(l1, l3))
    nets["policy"].precision = "fp16"
    with pytest.raises(ValueError):
        nets["policy"](x)


def test_bf16_memorises_512_positions(golden):
    feats, psd, vsd = golden
    x = torch.from_numpy(feats[:512]).to(DEV)
    rng = np.random.default_rng(8)
    tp = F.one_hot(torch.from_numpy(rng.integers(0, 81, 512)), 81).float().to(DEV)
    tv = torch.from_numpy(rng.choice([-1.0, 1.0], 512).astype(np.float32)).to(DEV)
    nets = _bf16_nets(psd, vsd)
    opts = {n: torch.optim.Adam(net.parameters(), lr=1e-3) for n, net in nets.items()}
    first = last = None
    for s in range(300):
        losses = [v.item() for v in _step(nets, opts, x, tp, tv)] if s in (0, 299) else _step(nets, opts, x, tp, tv)
        if s == 0:
            first = losses
        last = losses
    last = [float(v) for v in last]
    print("first", first, "last", last)
    assert last[0] < 0.5 * first[0], (first, last)
    assert last[1] < first[1], (first, last)


def test_bf16_eval_is_the_function_that_is_differentiated(golden):
    """eval mode: the no-grad path and the differentiated path (frozen BatchNorm) give the same bits in bf16 mode, and
    they are not the fp32 mode's"""
    feats, psd, _ = golden
    x = torch.from_numpy(feats[:64]).to(DEV)
    net = train.TrainablePolicyNet.from_state_dict(psd, device=DEV, precision="bf16").eval()
    with torch.no_grad():
        a = net(x)
    b = net(x)
    assert b.requires_grad and torch.equal(a, b.detach())
    net.precision = "fp32"
    with torch.no_grad():
        c = net(x)
    assert not torch.equal(a, c) and (a - c).abs().max().item() < 0.5


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_bf16_loop_closure(golden, tmp_path, capsys):
    from bokego_amd.engine import LeafEngine
    feats, psd, vsd = golden
    eng = LeafEngine(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw")),
                     max_batch=1024)
    try:
        local, _ = selfplay.self_play(selfplay.EngineEvaluator(eng), n_games=16, rollouts=32, max_turns=24, cap=1024,
                                      record_visits=1)
    finally:
        eng.close()
    rec = tmp_path / "r"
    selfplay.write_records(str(rec / "rank0"), local["games"], local["visits"])
    out = tmp_path / "out"
    train.main(["--records", str(rec), "--net", "both", "-c", os.path.join(GOLDEN, "policy_19.bkw"),
                os.path.join(GOLDEN, "value_synth.bkw"), "-e", "1", "-b", "64", "--lr", "1e-4", "--seed", "3",
                "--augment", "--precision", "bf16", "--out", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["precision"] == "bf16"
    assert line["epoch"] == 1 and line["positions"] > 0 and np.isfinite(line["policy_loss"])

    ckp, ckv = torch.load(out / "policy_1.pt"), torch.load(out / "value_1.pt")
    assert set(ckp) == {"model_state_dict", "optimizer_state_dict", "epoch"} and ckp["epoch"] == 1
    assert all(v.dtype in (torch.float32, torch.int64) for v in ckp["model_state_dict"].values())
    assert not torch.equal(ckp["model_state_dict"]["conv.3.weight"], psd["conv.3.weight"])
    assert ckp["model_state_dict"]["conv.1.num_batches_tracked"].item() == line["steps"]

    # the checkpoint is fp32 whatever trained it: the engine agrees with the trainable nets' fp32 eval()
    hp, hv = nnet.HipPolicyNet(ckp["model_state_dict"]), nnet.HipValueNet(ckv["model_state_dict"])
    tp = train.TrainablePolicyNet.from_state_dict(ckp, device=DEV).eval()
    tv = train.TrainableValueNet.from_state_dict(ckv, device=DEV).eval()
    assert tp.precision == tv.precision == "fp32"
    f32 = feats.astype(np.float32)
    with torch.no_grad():
        lg_t = tp(torch.from_numpy(f32).to(DEV)).cpu()
        va_t = tv(torch.from_numpy(f32).to(DEV)).cpu().reshape(-1)
    lg_e, va_e = hp(f32), hv(f32).reshape(-1)
    assert (lg_e - lg_t).abs().max().item() < 1e-4
    assert (va_e - va_t).abs().max().item() < 1e-4


def test_bf16_reinforce_epoch_is_deterministic_and_not_the_fp32_one(tmp_path, capsys):
    def run(name, precision):
        d = tmp_path / name
        d.mkdir()
        shutil.copy(os.path.join(GOLDEN, "policy_19.bkw"), d / "policy_0.bkw")
        reinforce.main(["-w", str(d), "-n", "1", "-b", "4", "--workers", "2", "--seed", "11", "-f", str(d / "stats.txt"),
                        "--precision", precision])
        capsys.readouterr()
        return torch.load(d / "policy_1.pt")["model_state_dict"]

    a, b, c = run("a", "bf16"), run("b", "bf16"), run("c", "fp32")
    assert set(a) == set(b) == set(c)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a if k.endswith(".weight"))

"""-m gpu: training on the MI355X (libbktrain.so + bokego_amd/train.py) against float64 torch on the CPU.

The float64 model is rebuilt here from the state_dict with torch ops (F.conv2d, F.batch_norm in train mode, ...), so
nothing in it shares code with what it checks."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bokego_amd import _trainlib as T
from bokego_amd import nnet, selfplay, train
from bokego_amd.bkw import load_bkw
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CONV = (0, 3, 6, 9, 12, 15, 18)
DEV = torch.device("cuda", 0)


def _seeded(shape, seed, zero_frac=0.2):
    """normal values of both signs with a share of exact zeros"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    a[torch.rand(shape, generator=g) < zero_frac] = 0
    return a.float()


def _bound_ok(got, ref, absref, factor=2e-6):
    """|got - ref| <= factor * sum|a*b| elementwise (absref: the same operation on |a| and |b| in float64)"""
    d = (got.double().cpu() - ref).abs()
    lim = factor * absref + 1e-30
    worst = (d / lim).max().item()
    assert worst <= 1.0, f"error {worst:.3g} x the bound"


# ---- the convolutions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 37, 256])
@pytest.mark.parametrize("cin,k", [(27, 5), (128, 3)])
def test_conv_kernels_against_float64(B, cin, k):
    seed = 1000 * B + k
    x, w, b = _seeded((B, cin, 9, 9), seed), _seeded((128, cin, k, k), seed + 1) * 0.1, _seeded((128,), seed + 2)
    dy = _seeded((B, 128, 9, 9), seed + 3)
    xd, wd, bd, dyd = x.double(), w.double(), b.double(), dy.double()
    pad = k // 2

    y = T.conv_forward(x.to(DEV), w.to(DEV), b.to(DEV))
    _bound_ok(y, F.conv2d(xd, wd, bd, padding=pad), F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=pad))

    dw, db = T.conv_wgrad(x.to(DEV), dy.to(DEV), w.shape)
    ref_dw = torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, padding=pad)
    _bound_ok(dw, ref_dw, torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), padding=pad))
    _bound_ok(db, dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3)))
    dw2, db2 = T.conv_wgrad(x.to(DEV), dy.to(DEV), w.shape)          # fixed-order sums: the same bits again
    assert torch.equal(dw, dw2) and torch.equal(db, db2)

    if cin == 128:
        dx = T.conv_dgrad(dy.to(DEV), w.to(DEV))
        _bound_ok(dx, torch.nn.grad.conv2d_input(xd.shape, wd, dyd, padding=pad),
                  torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), padding=pad))


def test_conv_refuses_what_it_does_not_support():
    x = torch.zeros((2, 27, 9, 9), device=DEV)
    with pytest.raises(ValueError):
        T.conv_forward(x, torch.zeros((128, 27, 4, 4), device=DEV))
    with pytest.raises(ValueError):
        T.conv_dgrad(torch.zeros((2, 128, 9, 9), device=DEV), torch.zeros((128, 27, 5, 5), device=DEV))
    with pytest.raises(ValueError):
        T.conv_forward(x.cpu(), torch.zeros((128, 27, 5, 5)))


# ---- BatchNorm2d + ReLU -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 37, 256])
def test_bn_relu_matches_torch_batchnorm(B):
    x = _seeded((B, 128, 9, 9), 7 + B, 0.05) * 3 + 0.5
    gamma, beta = _seeded((128,), 8, 0) * 0.5 + 1, _seeded((128,), 9, 0) * 0.2
    rm, rv = _seeded((128,), 10, 0) * 0.1, _seeded((128,), 11, 0).abs() + 0.5
    dy = _seeded((B, 128, 9, 9), 12, 0.1)

    ref = torch.nn.BatchNorm2d(128).double().train()
    with torch.no_grad():
        ref.weight.copy_(gamma), ref.bias.copy_(beta), ref.running_mean.copy_(rm), ref.running_var.copy_(rv)
    xd = x.double().requires_grad_(True)
    yd = torch.relu(ref(xd))
    yd.backward(dy.double())

    d_rm, d_rv, d_nbt = rm.to(DEV), rv.to(DEV), torch.tensor(0, dtype=torch.int64, device=DEV)
    y, mean, invstd = T.bn_relu_train(x.to(DEV), gamma.to(DEV), beta.to(DEV), d_rm, d_rv, d_nbt)
    assert (y.double().cpu() - yd.detach()).abs().max().item() < 2e-5
    assert (d_rm.double().cpu() - ref.running_mean).abs().max().item() < 1e-6
    assert ((d_rv.double().cpu() - ref.running_var).abs() / ref.running_var).max().item() < 1e-5
    assert d_nbt.item() == 1 == ref.num_batches_tracked.item()
    assert ((mean.double().cpu() - x.double().mean((0, 2, 3))).abs().max().item()) < 1e-5

    dx, dg, db = T.bn_relu_backward(dy.to(DEV), y, x.to(DEV), gamma.to(DEV), mean, invstd)
    for got, want in ((dx, xd.grad), (dg, ref.weight.grad), (db, ref.bias.grad)):
        assert (got.double().cpu() - want).norm() / want.norm() < 5e-5
    dx2, dg2, db2 = T.bn_relu_backward(dy.to(DEV), y, x.to(DEV), gamma.to(DEV), mean, invstd)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)

    ref.eval()                                         # eval mode: the running statistics the train step left
    ev = T.bn_relu_eval(x.to(DEV), gamma.to(DEV), beta.to(DEV), ref.running_mean.float().to(DEV),
                        ref.running_var.float().to(DEV))
    assert (ev.double().cpu() - torch.relu(ref(x.double()))).abs().max().item() < 2e-5


# ---- the float64 model, from the state_dict with torch ops ---------------------------------------------------------------
class Ref64:
    def __init__(self, sd, value):
        self.value = value
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
            h = F.conv2d(h, self.p[f"conv.{c}.weight"], self.p[f"conv.{c}.bias"], padding=2 if l == 0 else 1)
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


def _weight_of(name):
    return name.replace(".bias", ".weight")


@pytest.mark.parametrize("which", ["policy", "value"])
def test_one_training_step_against_float64(golden, which):
    feats, psd, vsd = golden
    sd = psd if which == "policy" else vsd
    cls = train.TrainablePolicyNet if which == "policy" else train.TrainableValueNet
    x = torch.from_numpy(feats[:256].astype(np.float32))
    tp, tv = _targets(256, 5)

    net = cls.from_state_dict(sd, device=DEV).train()
    ref = Ref64(net.state_dict(), which == "value")
    out = net(x.to(DEV))
    loss = train.policy_loss(out, tp.to(DEV)) if which == "policy" else train.value_loss(out, tv.to(DEV))
    loss.backward()
    rout = ref(x)
    rloss = train.policy_loss(rout, tp.double()) if which == "policy" else train.value_loss(rout, tv.double())
    rloss.backward()

    assert abs(loss.item() - rloss.item()) <= 1e-5 * abs(rloss.item())
    grads = {n: p.grad.double().cpu() for n, p in net.named_parameters()}
    assert set(grads) == set(ref.p)
    bad = []
    for n, g in grads.items():
        want = ref.p[n].grad
        if _zero_by_bn(n):
            lim = 1e-6 * grads[_weight_of(n)].norm()
            if not (g.norm() <= lim and want.norm() <= lim):
                bad.append((n, g.norm().item(), lim.item()))
        else:
            rel = ((g - want).norm() / want.norm()).item()
            if rel > 1e-4:
                bad.append((n, rel))
    assert not bad, bad
    # the running statistics the step left behind
    bufs = dict(net.named_buffers())
    for k, want in ref.buf.items():
        got = bufs[k].cpu()
        if k.endswith("num_batches_tracked"):
            assert got.item() == want.item() == 1, k
        else:
            assert (got.double() - want).norm() / want.norm() <= 1e-4, k


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


def test_steps_are_bit_deterministic(golden):
    feats, psd, vsd = golden
    x = torch.from_numpy(feats[:256]).to(DEV)
    tp, tv = (t.to(DEV) for t in _targets(256, 6))
    nets = {"policy": train.TrainablePolicyNet.from_state_dict(psd, device=DEV).train(),
            "value": train.TrainableValueNet.from_state_dict(vsd, device=DEV).train()}
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


def test_memorises_512_positions(golden):
    feats, psd, vsd = golden
    x = torch.from_numpy(feats[:512]).to(DEV)
    rng = np.random.default_rng(8)
    tp = F.one_hot(torch.from_numpy(rng.integers(0, 81, 512)), 81).float().to(DEV)
    tv = torch.from_numpy(rng.choice([-1.0, 1.0], 512).astype(np.float32)).to(DEV)
    nets = {"policy": train.TrainablePolicyNet.from_state_dict(psd, device=DEV).train(),
            "value": train.TrainableValueNet.from_state_dict(vsd, device=DEV).train()}
    opts = {n: torch.optim.Adam(net.parameters(), lr=1e-3) for n, net in nets.items()}
    first = last = None
    for s in range(300):
        losses = [v.item() for v in _step(nets, opts, x, tp, tv)] if s in (0, 299) else _step(nets, opts, x, tp, tv)
        if s == 0:
            first = losses
        last = losses
    last = [float(v) for v in last]
    assert last[0] < 0.5 * first[0], (first, last)
    assert last[1] < first[1], (first, last)


# ---- generate -> train -> generate ------------------------------------------------------------------------------------------
def test_loop_closure(golden, tmp_path, capsys):
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
                "--augment", "--out", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["epoch"] == 1 and line["positions"] > 0 and np.isfinite(line["policy_loss"])
    assert line["policy_checkpoint"] == str(out / "policy_1.pt") and line["value_checkpoint"] == str(out / "value_1.pt")

    ckp, ckv = torch.load(out / "policy_1.pt"), torch.load(out / "value_1.pt")
    assert set(ckp) == {"model_state_dict", "optimizer_state_dict", "epoch"} and ckp["epoch"] == 1
    # the weights moved and the BN counters count the steps
    assert not torch.equal(ckp["model_state_dict"]["conv.3.weight"], psd["conv.3.weight"])
    assert ckp["model_state_dict"]["conv.1.num_batches_tracked"].item() == line["steps"]

    # the engine takes the checkpoints through the existing .pt path and agrees with the trainable nets' eval()
    hp, hv = nnet.HipPolicyNet(ckp["model_state_dict"]), nnet.HipValueNet(ckv["model_state_dict"])
    tp = train.TrainablePolicyNet.from_state_dict(ckp, device=DEV).eval()
    tv = train.TrainableValueNet.from_state_dict(ckv, device=DEV).eval()
    f32 = feats.astype(np.float32)
    with torch.no_grad():
        lg_t = tp(torch.from_numpy(f32).to(DEV)).cpu()
        va_t = tv(torch.from_numpy(f32).to(DEV)).cpu().reshape(-1)
    lg_e, va_e = hp(f32), hv(f32).reshape(-1)
    assert lg_e.shape == (536, 81)
    assert (lg_e - lg_t).abs().max().item() < 1e-4
    assert (va_e - va_t).abs().max().item() < 1e-4

    # and the next generation plays on them
    eng = LeafEngine(ckp["model_state_dict"], ckv["model_state_dict"], max_batch=1024)
    try:
        nxt, _ = selfplay.self_play(selfplay.EngineEvaluator(eng), n_games=4, rollouts=16, max_turns=10, cap=1024)
    finally:
        eng.close()
    assert len(nxt["games"]) == 4 and all(len(g["moves"]) > 0 for g in nxt["games"].values())

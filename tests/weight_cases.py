"""Finite nets from the corners of the domain the engine accepts, with what float64 torch makes of them.

include/bokego_amd.h: the engine refuses non-finite weights and accepts every finite set with running_var + eps > 0.  The
nets the leaf kernels meet elsewhere in the suite (the two trained ones, test_gpu_parity._random_nets) all have BatchNorm
scales that are positive, of order one and nearly equal across channels; the cases here are what the folding and packing
code (bk_engine.cpp: pack_trunk, pack_trunk16, load_weights) has branches for and those nets never reach.

Shared by test_weight_domain_cpu.py (the reference alone: every case has the property its name claims, the reference's
own fp32 evaluation sits well inside every bound, no case sits near the f16x2 flag's threshold) and
test_gpu_weight_domain.py (both precisions of the engine against the same reference).  Everything is built in code from
seeds; the only fixture read is the goldens' feature planes.

Every case starts from a net of test_gpu_parity._random_nets' kind at gain 1 and, unless it says otherwise, changes
every trunk layer of both nets:

  neg_gamma         every third trunk gamma negated; bn.weight negative; every second lin_bn.weight negated
  zero_gamma        every fifth channel's gamma exactly 0: the channel is its bias alone
  tiny_var_small_w  running_var = 0 on channels 0, 16, ..., 1e-12 on channels 1, 17, ...; those channels' weights x 1e-3
  tiny_var_full_w   running_var = 0 on channels 0, 32, ..., weights untouched: activations reach ~1e12
  scale_invariant   per channel s = 2^k, k in -10..10: weight, bias and running_mean x s, running_var x s^2 (the same net up to eps)
  gamma_range       gamma x 2^U(-8, 3)
  zero_layer        all conv weights of trunk layer 3 are 0 (pack_trunk16: wmax == 0)
  tiny_layer        layer 2's conv weights x 2^-30, its running_var x 2^-60 (pack_trunk16: el at its upper clamp)
  big_heads         conv.21.weight x 40 (policy), lin2.weight x 60 (value): tanh saturates
  uniform_policy    policy conv.21.weight = 0, conv.21.bias = 0.25
  gain3             the base net at gain 3: |logit| ~ 170, the smallest probabilities ~ 1e-115
  huge_fold         one channel of the LAST trunk layer of each net folds to |w| = 2^31: running_var = 0, weights of 1 on that
                    channel and gamma = 6.5 * 2^20 (2^20 / sqrt(1e-5) alone is 2^28.3, which pack_trunk16's lower clamp
                    still holds inside fp16; the case is about the layer that does NOT fit, so gamma carries the other
                    2^2.7).  The channel's conv.21.weight is 2^-20, so the float64 logits stay below 1e6.

The reference is oracle/torch_ref.py's TorchPolicy / TorchValue in double on 32 rows: every 18th golden position (30 rows,
the empty board among them), a row of all-zero planes and a row of all-one planes.
"""
import collections
import functools
import os

import numpy as np

CONV = (0, 3, 6, 9, 12, 15, 18)
EPS = 1e-5
NAMES = ("neg_gamma", "zero_gamma", "tiny_var_small_w", "tiny_var_full_w", "scale_invariant", "gamma_range", "zero_layer",
         "tiny_layer", "big_heads", "uniform_policy", "gain3", "huge_fold")
FLOAT_PLANES = "gamma_range"               # the one case the GPU test feeds float32 planes; every other case gets uint8
HUGE_CHANNEL = 37                          # huge_fold: the channel of layer 6
FLAG_AT = 4094.0                           # the f16x2 kernel raises its flag at |activation| >= 65504 / 16

Reference = collections.namedtuple("Reference", "lg64 va64 pr64 lg32 va32 pr32 A")


def base(seed, gain=1.0):
    """-> (policy_sd, value_sd, rng): test_gpu_parity._random_nets' distribution, arrays that the caller may write to"""
    rng = np.random.default_rng(seed)

    def trunk():
        t = {}
        for l, c in enumerate(CONV):
            cin, k = (27, 5) if l == 0 else (128, 3)
            t[f"conv.{c}.weight"] = (rng.standard_normal((128, cin, k, k)) * gain / np.sqrt(cin * k * k)).astype(np.float32)
            t[f"conv.{c}.bias"] = (rng.standard_normal(128) * 0.1).astype(np.float32)
            t[f"conv.{c + 1}.weight"] = rng.uniform(0.5, 1.5, 128).astype(np.float32)
            t[f"conv.{c + 1}.bias"] = (rng.standard_normal(128) * 0.2).astype(np.float32)
            t[f"conv.{c + 1}.running_mean"] = (rng.standard_normal(128) * 0.2).astype(np.float32)
            t[f"conv.{c + 1}.running_var"] = rng.uniform(0.5, 2.0, 128).astype(np.float32)
        t["conv.21.weight"] = (rng.standard_normal((1, 128, 1, 1)) / np.sqrt(128)).astype(np.float32)
        t["conv.21.bias"] = (rng.standard_normal((1, 9, 9)) * 0.1).astype(np.float32)
        return t

    p, v = trunk(), trunk()
    v.update({"bn.weight": np.float32([1.3]), "bn.bias": np.float32([0.2]), "bn.running_mean": np.float32([-0.1]),
              "bn.running_var": np.float32([0.7]),
              "lin1.weight": (rng.standard_normal((64, 81)) / 9).astype(np.float32),
              "lin1.bias": (rng.standard_normal(64) * 0.1).astype(np.float32),
              "lin_bn.weight": rng.uniform(0.5, 1.5, 64).astype(np.float32),
              "lin_bn.bias": (rng.standard_normal(64) * 0.1).astype(np.float32),
              "lin_bn.running_mean": (rng.standard_normal(64) * 0.2).astype(np.float32),
              "lin_bn.running_var": rng.uniform(0.5, 2.0, 64).astype(np.float32),
              "lin2.weight": (rng.standard_normal((1, 64)) / 8).astype(np.float32), "lin2.bias": np.float32([0.05])})
    return p, v, rng


def _each_layer(p, v, f):
    """f(trunk, layer, conv index) over every trunk layer of both nets"""
    for t in (p, v):
        for l, c in enumerate(CONV):
            f(t, l, c)


def _neg_gamma(p, v, rng):
    def f(t, l, c):
        t[f"conv.{c + 1}.weight"][::3] *= -1
    _each_layer(p, v, f)
    v["bn.weight"] = np.float32([-1.3])
    v["lin_bn.weight"][::2] *= -1


def _zero_gamma(p, v, rng):
    def f(t, l, c):
        t[f"conv.{c + 1}.weight"][::5] = 0.0
    _each_layer(p, v, f)


def _tiny_var_small_w(p, v, rng):
    def f(t, l, c):
        t[f"conv.{c + 1}.running_var"][::16] = 0.0
        t[f"conv.{c + 1}.running_var"][1::16] = 1e-12
        t[f"conv.{c}.weight"][::16] *= 1e-3
        t[f"conv.{c}.weight"][1::16] *= 1e-3
    _each_layer(p, v, f)


def _tiny_var_full_w(p, v, rng):
    def f(t, l, c):
        t[f"conv.{c + 1}.running_var"][::32] = 0.0
    _each_layer(p, v, f)


def _scale_invariant(p, v, rng):
    def f(t, l, c):
        s = np.exp2(rng.integers(-10, 11, 128)).astype(np.float32)
        t[f"conv.{c}.weight"] *= s[:, None, None, None]
        t[f"conv.{c}.bias"] *= s
        t[f"conv.{c + 1}.running_mean"] *= s
        t[f"conv.{c + 1}.running_var"] *= s * s
    _each_layer(p, v, f)


def _gamma_range(p, v, rng):
    def f(t, l, c):
        t[f"conv.{c + 1}.weight"] *= np.exp2(rng.uniform(-8, 3, 128)).astype(np.float32)
    _each_layer(p, v, f)


def _zero_layer(p, v, rng):
    for t in (p, v):
        t[f"conv.{CONV[3]}.weight"][:] = 0.0


def _tiny_layer(p, v, rng):
    for t in (p, v):
        t[f"conv.{CONV[2]}.weight"] *= np.float32(2.0 ** -30)
        t[f"conv.{CONV[2] + 1}.running_var"] *= np.float32(2.0 ** -60)


def _big_heads(p, v, rng):
    p["conv.21.weight"] *= 40
    v["lin2.weight"] *= 60


def _uniform_policy(p, v, rng):
    p["conv.21.weight"][:] = 0.0
    p["conv.21.bias"][:] = 0.25


def _huge_fold(p, v, rng):
    c, m = CONV[6], HUGE_CHANNEL
    for t in (p, v):
        t[f"conv.{c + 1}.weight"][m] = 6.5 * 2.0 ** 20
        t[f"conv.{c + 1}.running_var"][m] = 0.0
        t[f"conv.{c}.weight"][m] = 1.0
        t["conv.21.weight"][0, m] = 2.0 ** -20


_BUILDERS = {"neg_gamma": (11, 1.0, _neg_gamma), "zero_gamma": (12, 1.0, _zero_gamma),
             "tiny_var_small_w": (13, 1.0, _tiny_var_small_w), "tiny_var_full_w": (14, 1.0, _tiny_var_full_w),
             "scale_invariant": (15, 1.0, _scale_invariant), "gamma_range": (16, 1.0, _gamma_range),
             "zero_layer": (17, 1.0, _zero_layer), "big_heads": (18, 1.0, _big_heads),
             "uniform_policy": (19, 1.0, _uniform_policy), "gain3": (20, 3.0, lambda p, v, rng: None),
             "tiny_layer": (21, 1.0, _tiny_layer), "huge_fold": (22, 1.0, _huge_fold)}
assert set(_BUILDERS) == set(NAMES)


@functools.lru_cache(maxsize=None)
def nets(name):
    """-> (policy_sd, value_sd) of the case, float32 arrays under the reference's names.  Shared: never written to."""
    seed, gain, change = _BUILDERS[name]
    p, v, rng = base(seed, gain)
    change(p, v, rng)
    for sd in (p, v):
        for a in sd.values():
            assert a.dtype == np.float32
            a.setflags(write=False)
    return p, v


@functools.lru_cache(maxsize=None)
def inputs():
    """uint8 [32, 27, 9, 9]: every 18th golden position, all-zero planes, all-one planes.  Shared: never written to."""
    from conftest import GOLDEN
    f = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"]
    assert len(f) == 536
    x = np.concatenate([f[::18], np.zeros((1, 27, 9, 9), f.dtype), np.ones((1, 27, 9, 9), f.dtype)]).astype(np.uint8)
    assert x.shape == (32, 27, 9, 9)
    x.setflags(write=False)
    return x


def planes(name):
    """the rows as the GPU test hands them to the engine for this case"""
    return inputs().astype(np.float32) if name == FLOAT_PLANES else inputs()


def big_planes():
    """float32 planes of 0, 70000, ... 490000 (exact): finite, and from 65520 on without an fp16 value -- for the golden nets"""
    x = inputs().astype(np.float32) * np.float32(70000.0)
    assert np.isfinite(x).all() and x.max() > 65520
    return x


@functools.lru_cache(maxsize=None)
def big_planes_reference():
    """the golden nets on big_planes() -> (float64 logits, float64 values, the reference's own fp32 logits and values)"""
    import torch

    from bokego_amd.bkw import load_bkw
    from conftest import GOLDEN
    from oracle.torch_ref import TorchPolicy, TorchValue
    pw, vw = load_bkw(os.path.join(GOLDEN, "policy_19.bkw")), load_bkw(os.path.join(GOLDEN, "value_synth.bkw"))
    x = torch.from_numpy(big_planes())
    return (TorchPolicy(pw).double()(x.double()).numpy(), TorchValue(vw).double()(x.double()).numpy(),
            TorchPolicy(pw)(x).numpy(), TorchValue(vw)(x).numpy())


def softmax64(lg):
    lg = np.asarray(lg, np.float64)
    e = np.exp(lg - lg.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 torch on the 32 rows -> Reference(logits, values, softmax64(logits), the reference's own fp32 logits, values
    and softmax, A = the largest post-ReLU trunk activation of both nets in float64)"""
    import torch

    from oracle.torch_ref import TorchPolicy, TorchValue
    p, v = nets(name)
    x = torch.from_numpy(inputs().astype(np.float32))
    P32, V32 = TorchPolicy(p), TorchValue(v)
    lg32t = P32(x)
    lg32, va32, pr32 = lg32t.numpy(), V32(x).numpy(), torch.softmax(lg32t, dim=1).numpy()
    P64, V64 = TorchPolicy(p).double(), TorchValue(v).double()     # float32 -> double is exact: the same weights
    xd = x.double()
    lg64, va64 = P64(xd).numpy(), V64(xd).numpy()
    A = 0.0
    with torch.no_grad():
        for net in (P64, V64):
            h = xd
            for blk in net.trunk.blocks:
                h = blk(h)
                A = max(A, h.max().item())
    out = Reference(lg64, va64, softmax64(lg64), lg32, va32, pr32, A)
    for a in out[:-1]:
        a.setflags(write=False)
    return out


def delta(name, tol_logit):
    """the logit bound of the case: tol_logit at the goldens' |logit| of 15, growing with the float64 logits"""
    return tol_logit * max(1.0, float(np.abs(reference(name).lg64).max()) / 15.0)


def folded(sd):
    """-> (scale [7, 128], wmax [7, 128]) in float64: the folded BatchNorm scale gamma / sqrt(var + eps) of every trunk
    channel, and the largest |w * scale| of the channel's folded conv weights (what pack_trunk / pack_trunk16 compute)"""
    scale, wmax = np.empty((7, 128)), np.empty((7, 128))
    for l, c in enumerate(CONV):
        g, var = sd[f"conv.{c + 1}.weight"].astype(np.float64), sd[f"conv.{c + 1}.running_var"].astype(np.float64)
        scale[l] = g / np.sqrt(var + EPS)
        wmax[l] = np.abs(sd[f"conv.{c}.weight"].astype(np.float64)).reshape(128, -1).max(1) * np.abs(scale[l])
    return scale, wmax


def f16_exponent(layer_wmax):
    """pack_trunk16's exponent for a layer whose largest folded |w| is layer_wmax -> (el before the clamp, el)"""
    el = int(np.floor(np.log2(32768.0 / layer_wmax))) if layer_wmax > 0 else 0
    return el, max(-14, min(el, 24))

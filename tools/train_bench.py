"""Training-step rate of bokego_amd/train.py on one MI355X: positions/s and achieved TFLOP/s.

    python tools/train_bench.py [--batches 256 1024] [--steps 20] [--warmup 5] [--out profiles/train_bench.json]
    python tools/train_bench.py --one 1024      # warm-up, then ONE step of both nets at B = 1024 (for rocprofv3)
    python tools/train_bench.py --precision bf16|both [...]     # the bf16 mixed-precision mode

A step is forward + loss + backward + Adam for the policy net, the value net, or both, on golden positions with
seeded targets; time is wall clock between device synchronisations, over --steps steps after --warmup.
FLOPs are algorithmic and count only the taps that land on the board (the project's convention):
forward 133.4 M, input gradient 6 x 20.48 M = 122.9 M, weight gradient 133.4 M: 389.7 MFLOP per position per net,
against the 157.3 TFLOP/s fp32-MFMA peak.  The heads (~0.02 % of the FLOPs) are not counted.
torch's own Conv2d + BatchNorm2d + ReLU trunk (MIOpen) on the same GPU is printed as a labelled yardstick.

--precision fp32 (the default) is the output described above, unchanged.  --precision bf16 times the same steps with the
trunk convolutions on bf16 operands; --precision both builds each set of nets once, warms both modes up and then
alternates them in one process (--rounds rounds of --steps steps each, the median round per mode), and prints the
ratio.  The FLOP count stays the algorithmic one.  A bf16 row carries TFLOP/s but no fraction of the fp32 peak: the
matrix pipe's dense bf16 peak is 2.5 PFLOP/s, and a bf16 step is bound by the staging of the fp32 operands, the fp32
BatchNorm / elementwise kernels and torch's ops, not by the matrix pipe.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bokego_amd import train  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
PEAK_TFLOPS = 157.3
BF16_NOTE = ("bf16 operands, fp32 accumulation; no fraction of the 157.3 TFLOP/s fp32-MFMA peak is given: the dense bf16 "
             "peak is 2.5 PFLOP/s, and the step is bound by operand staging, the fp32 BatchNorm / elementwise kernels and "
             "torch ops, not by the matrix pipe")


def _taps(k):
    h = k // 2
    one = sum(min(8, p + h) - max(0, p - h) + 1 for p in range(9))
    return one * one


FWD = 2 * 27 * 128 * _taps(5) + 6 * 2 * 128 * 128 * _taps(3)
DGRAD = 6 * 2 * 128 * 128 * _taps(3)
WGRAD = FWD
FLOP_PER_POS = FWD + DGRAD + WGRAD


def _data(B, dev):
    feats = np.load(os.path.join(GOLDEN, "features.npz"))["incremental"]
    idx = np.arange(B) % len(feats)
    rng = np.random.default_rng(B)
    x = torch.from_numpy(feats[idx]).to(dev)
    tp = F.one_hot(torch.from_numpy(rng.integers(0, 81, B)), 81).float().to(dev)
    tv = torch.from_numpy(rng.choice([-1.0, 1.0], B).astype(np.float32)).to(dev)
    return x, tp, tv


def _nets(which, dev, precision="fp32"):
    out = {}
    if which in ("policy", "both"):
        out["policy"] = train.TrainablePolicyNet.from_state_dict(train.load_weights(os.path.join(GOLDEN, "policy_19.bkw")),
                                                                 device=dev, precision=precision).train()
    if which in ("value", "both"):
        out["value"] = train.TrainableValueNet.from_state_dict(train.load_weights(os.path.join(GOLDEN, "value_synth.bkw")),
                                                               device=dev, precision=precision).train()
    return out


def _stepper(nets, x, tp, tv, lr=1e-4):
    opts = {n: torch.optim.Adam(net.parameters(), lr=lr) for n, net in nets.items()}

    def step():
        for n, net in nets.items():
            out = net(x)
            loss = train.policy_loss(out, tp) if n == "policy" else train.value_loss(out, tv)
            opts[n].zero_grad(set_to_none=True)
            loss.backward()
            opts[n].step()
    return step


def _torch_trunk(dev):
    """the same trunk on torch's Conv2d (MIOpen): the yardstick, not the product"""
    mods = []
    for l in range(7):
        k = 5 if l == 0 else 3
        mods += [torch.nn.Conv2d(27 if l == 0 else 128, 128, k, padding=k // 2), torch.nn.BatchNorm2d(128),
                 torch.nn.ReLU()]
    return torch.nn.Sequential(*mods, torch.nn.Conv2d(128, 1, 1)).to(dev).train()


def _time(step, steps, warmup, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps


def _row(which, B, dt, n, precision):
    row = {"what": f"train step, {which}", "batch": B, "ms_per_step": dt * 1e3, "positions_per_s": B / dt,
           "tflops": n * B * FLOP_PER_POS / dt / 1e12}
    if precision == "fp32":
        row["fraction_of_peak"] = row["tflops"] / PEAK_TFLOPS
    else:
        row["precision"] = precision
        row["note"] = BF16_NOTE
    return row


def _alternate(nets, step, steps, warmup, rounds, dev):
    """both modes warmed up, then `rounds` rounds of (fp32, bf16), `steps` steps each: the median round per mode"""
    def set_mode(m):
        for net in nets.values():
            net.precision = m
    times = {"fp32": [], "bf16": []}
    for m in times:
        set_mode(m)
        _time(step, 1, warmup, dev)
    for _ in range(rounds):
        for m in times:
            set_mode(m)
            times[m].append(_time(step, steps, 0, dev))
    return {m: float(np.median(v)) for m, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--one", type=int, default=None, help="warm up, then time one step of both nets at this batch")
    ap.add_argument("--out", default=None, help="also write the results (JSON) here")
    ap.add_argument("--precision", choices=["fp32", "bf16", "both"], default="fp32",
                    help="bf16: the mixed-precision mode; both: the two modes alternated in one process, with the ratio")
    ap.add_argument("--rounds", type=int, default=5, help="--precision both: rounds of --steps steps per mode")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    if args.one:
        if args.precision == "both":
            ap.error("--one takes --precision fp32 or bf16")
        x, tp, tv = _data(args.one, dev)
        step = _stepper(_nets("both", dev, args.precision), x, tp, tv)
        dt = _time(step, 1, 3, dev)
        line = {"one_step": "both", "batch": args.one, "ms": dt * 1e3}
        if args.precision != "fp32":
            line["precision"] = args.precision
        print(json.dumps(line))
        return

    rows = []
    for B in args.batches:
        x, tp, tv = _data(B, dev)
        for which in ("policy", "value", "both"):
            if args.precision == "both":
                nets = _nets(which, dev)
                dts = _alternate(nets, _stepper(nets, x, tp, tv), args.steps, args.warmup, args.rounds, dev)
                for m, dt in dts.items():
                    row = _row(which, B, dt, len(nets), m)
                    row["precision"] = m
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                row = {"what": f"train step, {which}: fp32 time / bf16 time", "batch": B,
                       "ratio": dts["fp32"] / dts["bf16"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue
            nets = _nets(which, dev, args.precision)
            dt = _time(_stepper(nets, x, tp, tv), args.steps, args.warmup, dev)
            row = _row(which, B, dt, len(nets), args.precision)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if not args.no_yardstick:
            net = _torch_trunk(dev)
            opt = torch.optim.Adam(net.parameters(), lr=1e-4)
            xf = x.float()

            def tstep():
                loss = -(tp * F.log_softmax(net(xf).reshape(-1, 81), 1)).sum(1).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            dt = _time(tstep, args.steps, args.warmup, dev)
            row = {"what": "YARDSTICK torch Conv2d/BatchNorm2d (MIOpen) trunk, policy-sized", "batch": B,
                   "ms_per_step": dt * 1e3, "positions_per_s": B / dt, "tflops": B * FLOP_PER_POS / dt / 1e12}
            rows.append(row)
            print(json.dumps(row), flush=True)
    meta = {"flop_per_position_per_net": FLOP_PER_POS, "forward": FWD, "input_gradient": DGRAD, "weight_gradient": WGRAD,
            "peak_tflops": PEAK_TFLOPS, "steps": args.steps, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(dev)}
    if args.precision != "fp32":
        meta.update({"precision": args.precision, "bf16_note": BF16_NOTE})
        if args.precision == "both":
            meta["rounds"] = args.rounds
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"meta": meta, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()

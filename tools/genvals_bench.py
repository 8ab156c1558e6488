"""Rate of the value-data generator (bokego_amd/genvals.py) on one MI355X: games/s of generate() with the device rules
(bkt_play_moves) against the host rules of reinforce.play_games, in the same process.

    python tools/genvals_bench.py [--games 4096 16384] [--reps 3] [--out profiles/genvals_bench.json]
    python tools/genvals_bench.py --one 4096      # warm-up, then ONE device-rules run at 4096 games (for rocprofv3)

Both policies are policy_19 (SL) and a seeded perturbation of it (RL).  One pass of G games (batch = G).  Per G: one
warm-up run of each rules mode, then --reps rounds that alternate device and host; the best of each is reported.
Times are wall clock between device synchronisations.  The per-ply split is one more run of each mode with a
synchronisation after each phase: 'engine' (both LeafEngine.eval_device calls), 'sampler' (bkt_sample_moves on three
slices, the masked logits, the move history), 'rules' (device: bkt_play_moves + the copy of the kept records; host:
bk_features_batch_u8, the planes upload, the moves download and bk_pos_play per game) and 'download' (the end of the
pass).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bokego_amd import genvals, reinforce, train  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")


def _policies():
    sl = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    rng = np.random.default_rng(5)
    rl = {k: (v * torch.from_numpy(1 + 0.05 * rng.standard_normal(tuple(v.shape))).to(v.dtype)
              if v.dtype.is_floating_point and "running" not in k else v) for k, v in sl.items()}
    return sl, rl


def _run(sl, rl, G, rules, seed, timing=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = genvals.generate(sl, rl, G, G, seed, rules=rules, timing=timing)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def bench_config(sds, G, reps):
    sl, rl = (reinforce.policy_engine(sd, 0, G) for sd in sds)
    try:
        for rules in ("device", "host"):
            _run(sl, rl, G, rules, 0)                                           # warm-up
        best = {"device": float("inf"), "host": float("inf")}
        rows = None
        for r in range(reps):
            for rules in ("device", "host"):
                out, dt = _run(sl, rl, G, rules, 1 + r)
                best[rules] = min(best[rules], dt)
                rows = len(out.rows)
        split = {}
        for rules in ("device", "host"):
            timing = {}
            _, dt = _run(sl, rl, G, rules, 100, timing)
            timing["total"] = dt
            split[rules] = {"seconds": timing,
                            "share": {k: v / dt for k, v in timing.items() if k != "total"}}
    finally:
        sl.close()
        rl.close()
    return {"games": G, "batch": G, "rows_kept": rows,
            "device_s": best["device"], "device_games_per_s": G / best["device"],
            "host_s": best["host"], "host_games_per_s": G / best["host"],
            "device_speedup": best["host"] / best["device"], "breakdown": split}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one", type=int, default=None, help="warm up, then one device-rules run at this many games")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sds = _policies()
    if args.one:
        sl, rl = (reinforce.policy_engine(sd, 0, args.one) for sd in sds)
        try:
            _run(sl, rl, args.one, "device", 0)
            out, dt = _run(sl, rl, args.one, "device", 1)
        finally:
            sl.close()
            rl.close()
        print(json.dumps({"one": args.one, "seconds": dt, "rows": len(out.rows)}))
        return
    out = {"device": torch.cuda.get_device_name(0), "configs": [bench_config(sds, G, args.reps) for G in args.games]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

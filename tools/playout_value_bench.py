"""What the one-launch random playouts (bkt_random_playouts) cost, on one MI355X.

    python tools/playout_value_bench.py [--games 4096 65536] [--reps 3] [--genmove-moves 10] [--out profiles/playout_value_bench.json]
    python tools/playout_value_bench.py --one 4096       # ONE pass of each path and nothing else (for rocprofv3)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/playout_value_bench.py --one 4096
    python tools/playout_value_bench.py --kernel-stats DIR [...]    # adds the kernels' per-call time from that run

playouts    G uniformly random eye-safe playouts from the empty board, through rollout.random_playouts (one launch and one
            bkt_area_score) and through the unchanged lock-step loop rollout.finish_games(engine=None, rules="device")
            (three launches and a history write per ply): the two paths alternated in one process after a warm-up, best
            of --reps each, wall clock between device synchronisations, downloads of the results included on both
            sides.  `ratio` = lock-step seconds / one-launch seconds; the gate at G = 4096 is ratio >= 1.0, recorded
            in that row as `gate` and `meets_gate`.
kernels     with --kernel-stats: calls and average ns per call of random_playouts_kernel, playout_step_kernel and
            sample_moves_kernel in one rocprofv3 --kernel-trace --stats run of --one (device time of the kernels: --one
            runs no warm-up pass, so that no other launch enters the averages).
genmove     ms/move of a 1600-rollout NativeMCTS genmove over the first --genmove-moves moves of a game: with
            playout_value=64 (policy_19, no value net) beside the same search on value_synth.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bokego_amd import nnet, reinforce, rollout  # noqa: E402
from bokego_amd.bkw import load_bkw  # noqa: E402
from bokego_amd.mcts_native import NativeMCTS, Position  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
GATE_GAMES, GATE_RATIO = 4096, 1.0                                   # the one-launch path is at least as fast as the loop
KERNELS = ("random_playouts_kernel", "playout_step_kernel", "sample_moves_kernel", "area_score_kernel")


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def bench_playouts(games, reps, seed):
    start = torch.from_numpy(reinforce.initial_positions(games)).cuda()
    paths = {"one_launch": lambda: rollout.random_playouts(start, seed),
             "one_launch_no_history": lambda: rollout.random_playouts(start, seed, history=False),
             "lock_step": lambda: rollout.finish_games(start, None, seed, rules="device")}
    for fn in paths.values():                                        # warm-up
        fn()
    best, fins = {}, {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            fin, dt = _timed(fn)
            if name not in best or dt < best[name]:
                best[name], fins[name] = dt, fin
    out = {"games": games}
    for name, dt in best.items():
        fin = fins[name]
        out[name] = {"seconds": dt, "playouts_per_s": games / dt, "plies_mean": float(fin.plies.mean()),
                     "plies_max": int(fin.plies.max()), "unfinished": int(fin.unfinished),
                     "black_wins": float((fin.score > 0).mean())}
    out["ratio"] = best["lock_step"] / best["one_launch"]
    out["ratio_no_history"] = best["lock_step"] / best["one_launch_no_history"]
    if games == GATE_GAMES:
        out["gate"] = GATE_RATIO
        out["meets_gate"] = bool(out["ratio"] >= GATE_RATIO)
    return out


def kernel_stats(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    out = {}
    for row in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in row["Name"]:
                out[k] = {"calls": int(row["Calls"]), "avg_ns": float(row["AverageNs"]), "total_ns": float(row.get("TotalDurationNs") or 0)}
    return out


def bench_genmove(moves, rollouts, playouts):
    pi = nnet.HipPolicyNet(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    val = nnet.HipValueNet(load_bkw(os.path.join(GOLDEN, "value_synth.bkw")))
    out = {"rollouts": rollouts, "moves": moves}
    for name, tree in (("value_synth", NativeMCTS(Position(), pi, val)),
                       (f"playout_value_{playouts}", NativeMCTS(Position(), pi, None, playout_value=playouts))):
        tree.rollout(100)                                            # warm-up
        per_move = []
        for _ in range(moves):
            t0 = time.perf_counter()
            tree.rollout(rollouts)
            tree.choose()
            per_move.append(time.perf_counter() - t0)
            if tree.root._terminal:
                break
        ev = tree.evaluator
        out[name] = {"ms_per_move": 1e3 * float(np.mean(per_move)), "ms_min": 1e3 * min(per_move), "ms_max": 1e3 * max(per_move),
                     "requests": int(ev.batches), "rows": int(ev.positions), "moves": tree._pool.moves(0)}
        tree.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--one", type=int, default=0, metavar="G")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    ap.add_argument("--genmove-moves", type=int, default=10)
    ap.add_argument("--genmove-rollouts", type=int, default=1600)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "playout_value_bench.json"))
    args = ap.parse_args()
    if args.one:
        start = torch.from_numpy(reinforce.initial_positions(args.one)).cuda()
        rollout.random_playouts(start, args.seed, history=False)
        rollout.finish_games(start, None, args.seed, rules="device")
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "playouts": [bench_playouts(g, args.reps, args.seed) for g in args.games]}
    for r in out["playouts"]:
        print(f"G={r['games']}: one launch {r['one_launch']['playouts_per_s']:.0f}/s ({r['one_launch']['seconds'] * 1e3:.1f} ms), "
              f"lock-step {r['lock_step']['playouts_per_s']:.0f}/s ({r['lock_step']['seconds'] * 1e3:.1f} ms), ratio {r['ratio']:.2f}",
              flush=True)
    if args.kernel_stats:
        out["kernels"] = kernel_stats(args.kernel_stats)
    if args.genmove_moves > 0:
        out["genmove"] = bench_genmove(args.genmove_moves, args.genmove_rollouts, args.playouts)
        print({k: (v["ms_per_move"] if isinstance(v, dict) else v) for k, v in out["genmove"].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "genmove"}))


if __name__ == "__main__":
    main()

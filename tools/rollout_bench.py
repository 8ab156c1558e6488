"""What playing games out to the end costs and what it changes (bokego_amd/rollout.py), on one MI355X.

    python tools/rollout_bench.py [--games 4096] [--reps 3] [--out profiles/rollout_bench.json]
    python tools/rollout_bench.py --one 4096     # warm-up, then ONE play_games(finish=True) (for rocprofv3)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rollout_bench.py --one 4096
    python tools/rollout_bench.py --kernel-stats DIR [...]    # adds the two rules kernels' per-call time from that run

reinforce   one play_games iteration of --games games (16 batches, policy_19 against itself): seconds and games/s of the
            71 sampled plies (finish=False), of the same iteration with finish=True, and of the finishing alone (the
            difference; best of --reps each, wall clock between device synchronisations); mean and max plies from ply
            71 to the end, the share of games unfinished at the default cap, and the share of games whose winner by the
            raw area at ply 71 differs from the winner of the finished board.
genvals     generate on --games games with and without finish: seconds, the plies, and the share of kept rows whose
            label differs.
kernels     with --kernel-stats: calls and average ns per call of playout_step_kernel and play_moves_kernel in one
            rocprofv3 --kernel-trace --stats run of --one, and their ratio (the step does strictly more work).
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

from bokego_amd import genvals, reinforce, rollout, train  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
WORKERS = 16


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _best(fn, reps):
    best = None
    for _ in range(reps):
        out, dt = _timed(fn)
        if best is None or dt < best[1]:
            best = (out, dt)
    return best


def bench_reinforce(eng, games, reps, seed):
    b = games // WORKERS
    play = lambda finish: reinforce.play_games(eng, eng, WORKERS, b, seed, iteration=1, finish=finish)  # noqa: E731
    play(True)                                                       # warm-up
    base, t_base = _best(lambda: play(False), reps)
    on, t_on = _best(lambda: play(True), reps)
    fin = on.finished
    return {"games": games, "sampled_plies": reinforce.POLICY_MAX_TURNS + 1,
            "seconds_sampled_plies": t_base, "games_per_s_sampled_plies": games / t_base,
            "seconds_with_finish": t_on, "games_per_s_with_finish": games / t_on,
            "seconds_finish_alone": t_on - t_base, "games_per_s_finish_alone": games / max(t_on - t_base, 1e-9),
            "games_played_out": int(len(on.finished_games)), "plies_to_end_mean": float(fin.plies.mean()),
            "plies_to_end_max": int(fin.plies.max()), "max_plies_cap": rollout.MAX_PLIES,
            "share_unfinished_at_cap": fin.unfinished / len(fin.plies),
            "share_winner_differs_from_raw_area": float((on.black_wins != base.black_wins).mean()),
            "black_wins_raw": int(base.black_wins.sum()), "black_wins_finished": int(on.black_wins.sum())}


def bench_genvals(eng, games, reps, seed):
    gen = lambda finish: genvals.generate(eng, eng, games, games, seed, finish=finish)  # noqa: E731
    gen(True)
    a, t_a = _best(lambda: gen(False), reps)
    b, t_b = _best(lambda: gen(True), reps)
    differs = np.array([x[4] != y[4] for x, y in zip(a.rows, b.rows)])
    return {"games": games, "rows": len(a.rows), "seconds": t_a, "games_per_s": games / t_a,
            "seconds_with_finish": t_b, "games_per_s_with_finish": games / t_b,
            "share_label_differs_from_raw_area": float(differs.mean()) if len(differs) else 0.0,
            "share_winner_differs_all_games": float(((a.score > 0) != (b.score > 0)).mean())}


def kernel_stats(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    out = {}
    for r in csv.DictReader(open(files[0])):
        for name in ("playout_step_kernel", "play_moves_kernel"):
            if name in r["Name"]:
                out[name] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])}
    if len(out) == 2:
        out["step_over_play_moves"] = out["playout_step_kernel"]["average_ns"] / out["play_moves_kernel"]["average_ns"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--one", type=int, default=None, metavar="GAMES")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_bench.json"))
    args = ap.parse_args()
    games = args.one or args.games
    if games % WORKERS:
        ap.error(f"the number of games must be a multiple of {WORKERS}")
    eng = reinforce.policy_engine(train.load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, games)
    try:
        if args.one:
            b = games // WORKERS
            reinforce.play_games(eng, eng, WORKERS, b, args.seed, iteration=0, finish=True)
            torch.cuda.synchronize()
            reinforce.play_games(eng, eng, WORKERS, b, args.seed, iteration=1, finish=True)
            torch.cuda.synchronize()
            return
        out = {"device": torch.cuda.get_device_name(0), "policy": "tests/golden/policy_19.bkw", "reps": args.reps,
               "reinforce": bench_reinforce(eng, games, args.reps, args.seed),
               "genvals": bench_genvals(eng, games, args.reps, args.seed)}
    finally:
        eng.close()
    if args.kernel_stats:
        out["kernels"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

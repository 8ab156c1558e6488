"""What RAVE in the native tree search and its two-sided AMAF reduction (bkt_amaf_counts_sides) cost and whether they
win games, on one MI355X.  Nothing here has a threshold: the figures are recorded.  By tools/pattern_playout_bench.py's
protocol: a warm-up, the paths alternated in one process, best of --reps.

    python tools/rave_bench.py kernel  [--records 1024] [--playouts 64] [--reps 3]
    python tools/rave_bench.py genmove [--genmoves 8] [--rollouts 400] [--playouts 64] [--rave 16] [--reps 3]
    python tools/rave_bench.py match --rave K [--games 100] [--rollouts 400] [--playouts 64] [--opening-plies 4] [--seed 1]
    (each with [--out profiles/rave_bench.json]: a part replaces its own entry of that file and leaves the others;
     genmove and match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

kernel      bkt_amaf_counts_sides against bkt_amaf_counts on the same --records x --playouts histories, from the empty board
            and from ply 40 of policy_19 games, by HIP events, alternated, best of --reps; `ratio` = sides / one side.  Both
            read the same bytes.
genmove     ms per move of --genmoves moves of a net-free search from the empty board, --rollouts rollouts a move, with
            playout_rave=--rave and without it: two trees alternated move by move (each plays its own game), the whole
            run --reps times, best mean.  `ratio` = with / without.
match       --games games, colours alternated, --rollouts rollouts a move: the in-process GTP engine of
            `gtp --playout-value N --playout-prior 1 --playout-rave K` against the same engine without --playout-rave.  Both
            are deterministic, so every pair of games starts from --opening-plies seeded random moves (match.random_opening),
            the pair sharing its opening.  Wins and ms/move of both; 100 games resolve about +-10 points, so a result within
            40..60 is recorded as "no difference shown".
A part that did not run reads "not measured".  Run the parts one process each, every one under its own time limit.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from bokego_amd import _trainlib as T  # noqa: E402
from bokego_amd import lockstep as L  # noqa: E402
from bokego_amd import match, reinforce, rollout  # noqa: E402
from bokego_amd.mcts_native import NativeMCTS, Position  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
PARTS = ("kernel", "genmove", "match")


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_kernel(recs, playouts, reps, seed):
    run = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", history=True)
    won, moves = run.won.to(torch.uint8).reshape(-1), run.moves
    paths = {"sides": lambda: T.amaf_counts_sides(moves, won, len(recs), playouts),
             "one_side": lambda: T.amaf_counts(moves, won, len(recs), playouts)}
    two, one = paths["sides"](), paths["one_side"]()                  # warm-up, and the same integers
    assert torch.equal(two[0][:, 0], one[0]) and torch.equal(two[1][:, 0], one[1])
    best = {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            ms = _event_ms(fn)
            best[name] = min(ms, best.get(name, ms))
    return {"records": len(recs), "playouts": playouts, "rows": len(recs) * playouts, "max_plies": int(moves.shape[1]),
            "history_bytes": int(moves.numel() * 2), "sides_ms": best["sides"], "one_side_ms": best["one_side"],
            "ratio": best["sides"] / best["one_side"]}


def part_kernel(args):
    from amaf_prior_bench import positions_at_ply
    from bokego_amd.train import load_weights
    eng = reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 4096)
    try:
        pos, _ = positions_at_ply(eng, 4096, 202)
    finally:
        eng.close()
    starts = {"empty_board": torch.from_numpy(reinforce.initial_positions(args.records)).cuda(),
              "ply_40": pos[:args.records].contiguous()}
    out = {}
    for name, recs in starts.items():
        out[name] = r = bench_kernel(recs, args.playouts, args.reps, args.seed)
        print(f"{name}: {r['records']} x {r['playouts']}: sides {r['sides_ms']:.3f} ms, one side {r['one_side_ms']:.3f} ms, "
              f"x{r['ratio']:.3f}", flush=True)
    return out


def part_genmove(args):
    kinds = {"rave": {"playout_rave": args.rave}, "plain": {}}
    best = {}
    for _ in range(args.reps):
        trees = {k: NativeMCTS(Position(), None, None, playout_value=args.playouts, playout_prior=1.0, playout_seed=args.seed,
                               playout_rules=args.rules, **kw)
                 for k, kw in kinds.items()}
        ms = {k: [] for k in kinds}
        for t in trees.values():
            t.rollout(8)                                             # warm-up
        for _ in range(args.genmoves):                               # alternated, move by move
            for k, t in trees.items():
                if args.rules == "device":
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                t.rollout(args.rollouts)
                t.choose()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for k, t in trees.items():
            t.close()
            mean = float(np.mean(ms[k]))
            if k not in best or mean < best[k]["ms_per_move"]:
                best[k] = {"ms_per_move": mean, "ms_each": ms[k]}
    out = {"rollouts": args.rollouts, "playouts": args.playouts, "playout_rave": args.rave, "genmoves": args.genmoves,
           "rave": best["rave"], "plain": best["plain"], "ratio": best["rave"]["ms_per_move"] / best["plain"]["ms_per_move"]}
    print(f"net-free genmove at {args.rollouts} rollouts: with playout_rave={args.rave:g} {out['rave']['ms_per_move']:.2f} ms/move, "
          f"without {out['plain']['ms_per_move']:.2f}, x{out['ratio']:.3f}", flush=True)
    return out


def part_match(args):
    from bokego_amd.gtp import NativeGTP

    def engine(name, **more):
        return match.InProcessEngine(NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=args.rollouts,
                                               playout_value=args.playouts, playout_prior=1.0, playout_rules=args.rules, **more),
                                     name=name)

    a, b = engine("rave", playout_rave=args.rave), engine("plain")
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["rave_wins"]
    share = 100.0 * wins / args.games
    res.update(playout_rave=args.rave, rollouts=args.rollouts, playouts=args.playouts, opening_plies=args.opening_plies,
               seed=args.seed, verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("RAVE wins beyond the margin" if share > 60.0 else "RAVE loses beyond the margin"))
    print(f"match k={args.rave:g}: RAVE {wins} : {res['plain_wins']} plain over {args.games} games -- {res['verdict']}; ms/move "
          f"{res['ms_per_move']['rave']:.2f} / {res['ms_per_move']['plain']:.2f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--genmoves", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--rave", type=float, default=16.0, metavar="K")
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--rules", choices=("device", "host"), default="device")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rave_bench.json"))
    args = ap.parse_args()
    out = {"kernel": "not measured", "genmove": "not measured", "match": {f"k={k}": "not measured" for k in (4, 16, 64)}}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0) if args.rules == "device" else "none (host rules: a dry run)"
    if args.part == "match":
        key = f"k={args.rave:g}" + ("" if args.seed == ap.get_default("seed") else f",seed={args.seed}")   # (another seed: other openings)
        out["match"][key] = part_match(args)
    else:
        out[args.part] = (part_kernel if args.part == "kernel" else part_genmove)(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

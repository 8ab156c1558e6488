"""What the pattern-weighted playouts (bkt_pattern_playouts) cost and what they buy, on one MI355X.

    python tools/pattern_playout_bench.py [--games 4096 65536] [--reps 3] [--fit-games 4096] [--quality-games 4096]
                                          [--playouts 64] [--out profiles/pattern_playout_bench.json]

fit         the table every other part uses: patterns.counts / symmetrise / weights on --fit-games policy_19 games from the
            empty board played to the end with seed A (--fit-seed), and the seconds the games and the counting took.
playouts    G playouts from the empty board through rollout.random_playouts with that table (one bkt_pattern_playouts
            launch and one bkt_area_score), through the same call without a table (bkt_random_playouts) and through the
            lock-step loop rollout.finish_games(engine=None, rules="device"): the three alternated in one process after a
            warm-up, best of --reps each, wall clock between device synchronisations, downloads included on every side.
            `ratio_lock_step` = lock-step seconds / pattern seconds; the gate at G = 4096 is >= 1.0 (`gate`, `meets_gate`).
            `ratio_uniform` = pattern seconds / uniform seconds, the price of the weighted draw: recorded, no threshold.
quality     --quality-games policy_19 games with seed B (--quality-seed) played to the end; at their ply-40 positions
            (games at least 41 plies long), how often the sign of playout_value at N = --playouts agrees with the winner of
            the finished game, for the uniform playouts and for the fitted table (a value of 0 agrees with nobody and is
            counted in `ties`).  Recorded, no threshold.
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

from bokego_amd import _trainlib as T  # noqa: E402
from bokego_amd import lockstep as L  # noqa: E402
from bokego_amd import patterns, reinforce, rollout  # noqa: E402
from bokego_amd.train import load_weights  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
GATE_GAMES, GATE_RATIO = 4096, 1.0                                   # one launch is at least as fast as the lock-step loop
QUALITY_PLY = 40


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def policy_games(eng, games, seed):
    start = reinforce.initial_positions(games)
    return start, rollout.finish_games(start, eng, seed)


def fit_table(eng, games, seed):
    (start, fin), t_games = _timed(lambda: policy_games(eng, games, seed))
    (seen, played), t_counts = _timed(lambda: patterns.counts(start, fin.moves))
    table = patterns.PatternTable(patterns.weights(*patterns.symmetrise(seen, played)))
    info = {"games": games, "seed": seed, "policy": "policy_19.bkw", "seconds_games": t_games, "seconds_counts": t_counts,
            "moves": int(played.sum()), "playable_points": int(seen.sum()), "patterns_seen": int((seen > 0).sum()),
            "weight_min": int(table.array.min()), "weight_max": int(table.array.max()),
            "weight_of_unseen": int(patterns.weights([0], [0])[0])}
    return table, info


def bench_playouts(games, reps, seed, table):
    start = torch.from_numpy(reinforce.initial_positions(games)).cuda()
    paths = {"pattern": lambda: rollout.random_playouts(start, seed, patterns=table),
             "uniform": lambda: rollout.random_playouts(start, seed),
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
    out["ratio_lock_step"] = best["lock_step"] / best["pattern"]
    out["ratio_uniform"] = best["pattern"] / best["uniform"]
    if games == GATE_GAMES:
        out["gate"] = GATE_RATIO
        out["meets_gate"] = bool(out["ratio_lock_step"] >= GATE_RATIO)
    return out


def bench_quality(eng, games, seed, playouts, value_seed, table):
    start, fin = policy_games(eng, games, seed)
    rows = np.nonzero(fin.over & (fin.plies > QUALITY_PLY))[0]
    pos = torch.from_numpy(start[rows]).cuda()
    hist = torch.from_numpy(fin.moves[rows, :QUALITY_PLY].astype(np.int32)).cuda()
    status = torch.zeros(len(rows), dtype=torch.int32, device=pos.device)
    for k in range(QUALITY_PLY):
        status |= T.playout_step(pos, hist[:, k].contiguous(), None, None, None)
    assert not status.any().item()
    mover_wins = (torch.from_numpy(fin.score[rows] > 0).cuda() == L.black_to_move(pos)).cpu().numpy()
    out = {"games": games, "seed": seed, "ply": QUALITY_PLY, "positions": int(len(rows)), "playouts": playouts,
           "value_seed": value_seed, "mover_wins": float(mover_wins.mean())}
    for name, t in (("uniform", None), ("pattern", table)):
        v, dt = _timed(lambda: rollout.playout_value(pos, playouts, value_seed, patterns=t))
        out[name] = {"agreement": float(((v > 0) == mover_wins)[v != 0].sum() / len(rows)), "ties": float((v == 0).mean()),
                     "mean_abs_value": float(np.abs(v).mean()), "seconds": dt}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fit-games", type=int, default=4096)
    ap.add_argument("--fit-seed", type=int, default=101)
    ap.add_argument("--quality-games", type=int, default=4096)
    ap.add_argument("--quality-seed", type=int, default=202)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--table-out", default=None, metavar="FILE", help="also save the fitted table")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pattern_playout_bench.json"))
    args = ap.parse_args()
    eng = reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0,
                                  min(max(args.fit_games, args.quality_games, 1), 4096))
    try:
        table, fit = fit_table(eng, args.fit_games, args.fit_seed)
        print(f"fit: {fit['moves']} moves of {fit['games']} games, {fit['patterns_seen']} patterns seen, "
              f"{fit['seconds_games']:.2f} s games + {fit['seconds_counts']:.2f} s counts", flush=True)
        if args.table_out:
            table.save(args.table_out)
        out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "fit": fit,
               "playouts": [bench_playouts(g, args.reps, args.seed, table) for g in args.games]}
        for r in out["playouts"]:
            print(f"G={r['games']}: pattern {r['pattern']['playouts_per_s']:.0f}/s ({r['pattern']['seconds'] * 1e3:.1f} ms), "
                  f"uniform {r['uniform']['playouts_per_s']:.0f}/s, lock-step {r['lock_step']['playouts_per_s']:.0f}/s, "
                  f"x{r['ratio_lock_step']:.2f} the loop, x{r['ratio_uniform']:.2f} the uniform kernel's time", flush=True)
        if args.quality_games > 0:
            out["quality"] = q = bench_quality(eng, args.quality_games, args.quality_seed, args.playouts, args.seed, table)
            print(f"quality at ply {q['ply']} ({q['positions']} positions, N={q['playouts']}): uniform "
                  f"{q['uniform']['agreement']:.4f}, pattern {q['pattern']['agreement']:.4f}", flush=True)
        out["match"] = "not measured"
    finally:
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

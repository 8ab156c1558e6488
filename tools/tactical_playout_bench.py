"""What the tactical playouts (bkt_tactical_playouts) cost and what they buy, on one MI355X.

    python tools/tactical_playout_bench.py [--games 4096 65536] [--reps 3] [--fit-games 4096] [--quality-games 4096]
                                           [--playouts 64] [--out profiles/tactical_playout_bench.json]

The protocol is tools/pattern_playout_bench.py's: the same seeds, games, alternation and best of --reps.

fit         the pattern table as that tool fits it (--fit-games policy_19 games from the empty board, seed --fit-seed), then
            the tactics table on top of it from the same games (tactics.counts / weights), and a second tactics table fitted
            without patterns for the "tactics alone" figure; the 64 fitted entries are recorded (`tactics`, `tactics_alone`).
playouts    G playouts from the empty board through rollout.random_playouts with both tables (one bkt_tactical_playouts
            launch and one bkt_area_score), with the pattern table only (bkt_pattern_playouts), with no table
            (bkt_random_playouts) and through the lock-step loop rollout.finish_games(engine=None, rules="device"): the four
            alternated in one process after a warm-up, best of --reps each, wall clock between device synchronisations.
            `ratio_lock_step` = lock-step seconds / tactical seconds; the gate at G = 4096 is >= 1.0 (`gate`, `meets_gate`).
            `ratio_patterns` = tactical seconds / pattern seconds, the price of the tactical weights: recorded, no threshold.
quality     --quality-games policy_19 games with seed --quality-seed played to the end; at their ply-40 positions, how often
            the sign of playout_value at N = --playouts agrees with the winner of the finished game, for uniform playouts,
            patterns, tactics alone and both together (a value of 0 agrees with nobody: `ties`).  Recorded, no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bokego_amd import _trainlib as T  # noqa: E402
from bokego_amd import lockstep as L  # noqa: E402
from bokego_amd import patterns, reinforce, rollout, tactics  # noqa: E402
from bokego_amd.train import load_weights  # noqa: E402
from pattern_playout_bench import GATE_GAMES, GATE_RATIO, GOLDEN, QUALITY_PLY, _timed, policy_games  # noqa: E402


def fit_tables(eng, games, seed):
    """The pattern table as pattern_playout_bench.fit_table makes it, and the two tactics tables, from the same games."""
    (start, fin), t_games = _timed(lambda: policy_games(eng, games, seed))
    (seen, played), t_counts = _timed(lambda: patterns.counts(start, fin.moves))
    table = patterns.PatternTable(patterns.weights(*patterns.symmetrise(seen, played)))
    out = {"patterns": table,
           "info": {"games": games, "seed": seed, "policy": "policy_19.bkw", "seconds_games": t_games,
                    "seconds_pattern_counts": t_counts, "moves": int(played.sum()), "patterns_seen": int((seen > 0).sum())}}
    out.update(fit_tactics(start, fin.moves, table))
    return out


def fit_tactics(start, moves, table):
    out = {}
    for name, pat in (("tactics", table), ("tactics_alone", None)):
        (mass, played), dt = _timed(lambda: tactics.counts(start, moves, pat))
        out[name] = tactics.TacticTable(tactics.weights(mass, played))
        out[name + "_info"] = {"seconds_counts": dt, "played": played.tolist(), "mass": [round(float(m), 3) for m in mass],
                               "entries": out[name].array.tolist()}
    return out


def bench_playouts(games, reps, seed, table, tac):
    start = torch.from_numpy(reinforce.initial_positions(games)).cuda()
    paths = {"tactical": lambda: rollout.random_playouts(start, seed, patterns=table, tactics=tac),
             "pattern": lambda: rollout.random_playouts(start, seed, patterns=table),
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
    out["ratio_lock_step"] = best["lock_step"] / best["tactical"]
    out["ratio_patterns"] = best["tactical"] / best["pattern"]
    if games == GATE_GAMES:
        out["gate"] = GATE_RATIO
        out["meets_gate"] = bool(out["ratio_lock_step"] >= GATE_RATIO)
    return out


def bench_quality(eng, games, seed, playouts, value_seed, tables):
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
    for name, pat, tac in (("uniform", None, None), ("pattern", tables["patterns"], None),
                           ("tactics_alone", None, tables["tactics_alone"]),
                           ("pattern_and_tactics", tables["patterns"], tables["tactics"])):
        v, dt = _timed(lambda: rollout.playout_value(pos, playouts, value_seed, patterns=pat, tactics=tac))
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
    ap.add_argument("--tactics-out", default=None, metavar="FILE", help="also save the fitted tactics table")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tactical_playout_bench.json"))
    args = ap.parse_args()
    eng = reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0,
                                  min(max(args.fit_games, args.quality_games, 1), 4096))
    try:
        tables = fit_tables(eng, args.fit_games, args.fit_seed)
        print(f"fit: {tables['info']['moves']} moves of {args.fit_games} games", flush=True)
        print(tactics.show(tables["tactics"]), flush=True)
        if args.tactics_out:
            tables["tactics"].save(args.tactics_out)
        out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
               "fit": dict(tables["info"], tactics=tables["tactics_info"], tactics_alone=tables["tactics_alone_info"]),
               "playouts": [bench_playouts(g, args.reps, args.seed, tables["patterns"], tables["tactics"])
                            for g in args.games]}
        for r in out["playouts"]:
            print(f"G={r['games']}: tactical {r['tactical']['playouts_per_s']:.0f}/s ({r['tactical']['seconds'] * 1e3:.1f} ms), "
                  f"pattern {r['pattern']['playouts_per_s']:.0f}/s, uniform {r['uniform']['playouts_per_s']:.0f}/s, lock-step "
                  f"{r['lock_step']['playouts_per_s']:.0f}/s, x{r['ratio_lock_step']:.2f} the loop, x{r['ratio_patterns']:.2f} "
                  "the pattern kernel's time", flush=True)
        if args.quality_games > 0:
            out["quality"] = q = bench_quality(eng, args.quality_games, args.quality_seed, args.playouts, args.seed, tables)
            print(f"quality at ply {q['ply']} ({q['positions']} positions, N={q['playouts']}): " +
                  ", ".join(f"{k} {q[k]['agreement']:.4f}" for k in ("uniform", "pattern", "tactics_alone",
                                                                     "pattern_and_tactics")), flush=True)
        out["match"] = "not measured"
    finally:
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

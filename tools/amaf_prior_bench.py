"""What the AMAF counts of the playouts (bkt_amaf_counts, rollout.playout_amaf) cost and what their prior knows, on
one MI355X.  Nothing here has a threshold: the figures are recorded.

    python tools/amaf_prior_bench.py [--records 1024] [--playouts 64] [--reps 3] [--fit-games 4096] [--quality-games 4096]
                                     [--genmoves 4] [--rollouts 400] [--out profiles/amaf_prior_bench.json]

time        rollout.playout_amaf against rollout.playout_value on the same --records records x --playouts playouts, from the
            empty board and from ply 40 of policy_19 games: the two alternated in one process after a warm-up, best of --reps
            each, wall clock between device synchronisations, downloads included on both sides.  `ratio` = amaf seconds /
            value seconds: the price of the history and the reduction.  `reduction_ms`: the bkt_amaf_counts call alone on that
            history, by HIP events, best of --reps.
quality     the ply-40 positions of --quality-games policy_19 games with seed B (--quality-seed; games at least 41 plies long
            whose move 40 is no pass): the share in which the move the policy played there is the top-1 of
            amaf_prior(playout_amaf(N = --playouts)), and the share in which it is among the top-5 -- for uniform playouts and
            for a pattern table fitted as tools/pattern_playout_bench.py fits it (--fit-games games, seed A), and beside them
            what a uniform prior over the legal points gets on the same positions (1 / L and min(5, L) / L on average).
genmove     ms per move of --genmoves moves of a search without any network from the empty board:
            NativeMCTS(playout_value=--playouts, playout_prior=1.0), --rollouts rollouts a move.
match       not measured here (python -m bokego_amd.match --playout-value 64 --playout-prior 1 plays it).
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
from bokego_amd import reinforce, rollout  # noqa: E402
from bokego_amd.mcts_native import NativeMCTS, Position  # noqa: E402
from bokego_amd.train import load_weights  # noqa: E402
from pattern_playout_bench import GOLDEN, QUALITY_PLY, _timed, fit_table, policy_games  # noqa: E402


def positions_at_ply(eng, games, seed):
    """The ply-40 records of the policy games that got there and played a point next -> (records on the device, that move)."""
    start, fin = policy_games(eng, games, seed)
    rows = np.nonzero(fin.over & (fin.plies > QUALITY_PLY) & (fin.moves[:, QUALITY_PLY] >= 0))[0]
    pos = torch.from_numpy(start[rows]).cuda()
    hist = torch.from_numpy(fin.moves[rows, :QUALITY_PLY].astype(np.int32)).cuda()
    status = torch.zeros(len(rows), dtype=torch.int32, device=pos.device)
    for k in range(QUALITY_PLY):
        status |= T.playout_step(pos, hist[:, k].contiguous(), None, None, None)
    assert not status.any().item()
    return pos, fin.moves[rows, QUALITY_PLY].astype(np.int64)


def bench_time(recs, playouts, reps, seed):
    paths = {"amaf": lambda: rollout.playout_amaf(recs, playouts, seed),
             "value": lambda: rollout.playout_value(recs, playouts, seed)}
    for fn in paths.values():                                        # warm-up
        fn()
    best, last = {}, {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            last[name], dt = _timed(fn)
            best[name] = min(dt, best.get(name, dt))
    assert np.array_equal(last["amaf"].value, last["value"])
    # the reduction alone, on the history of these playouts
    run = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", history=True)
    won, moves = run.won.to(torch.uint8).reshape(-1), run.moves
    ms = []
    for _ in range(reps + 1):                                        # the first is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        T.amaf_counts(moves, won, len(recs), playouts)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"records": len(recs), "playouts": playouts, "rows": len(recs) * playouts, "max_plies": int(moves.shape[1]),
            "amaf_seconds": best["amaf"], "value_seconds": best["value"], "ratio": best["amaf"] / best["value"],
            "reduction_ms": min(ms[1:]), "history_bytes": int(moves.numel() * 2),
            "plies_mean": float((moves > rollout.MOVE_NONE).sum(1).float().mean().item())}


def bench_quality(pos, played, playouts, seed, table):
    recs = pos.cpu().numpy()
    legal = rollout.legal_host(recs)
    n_legal = legal.sum(1)
    assert legal[np.arange(len(recs)), played].all()
    out = {"ply": QUALITY_PLY, "positions": int(len(recs)), "playouts": playouts, "value_seed": seed,
           "legal_points_mean": float(n_legal.mean()),
           "uniform_prior": {"top1": float((1.0 / n_legal).mean()), "top5": float((np.minimum(5, n_legal) / n_legal).mean())}}
    for name, t in (("uniform_playouts", None), ("pattern_playouts", table)):
        amaf, dt = _timed(lambda: rollout.playout_amaf(pos, playouts, seed, patterns=t))
        prior = rollout.amaf_prior(recs, amaf)
        order = np.argsort(-prior, 1, kind="stable")
        out[name] = {"top1": float((order[:, 0] == played).mean()), "top5": float((order[:, :5] == played[:, None]).any(1).mean()),
                     "mean_prior_of_the_move": float(prior[np.arange(len(recs)), played].mean()), "seconds": dt}
    return out


def bench_genmove(moves, rollouts, playouts, seed):
    tree = NativeMCTS(Position(), None, None, playout_value=playouts, playout_prior=1.0, playout_seed=seed)
    tree.rollout(8)                                                  # warm-up
    ms, played = [], []
    for _ in range(moves):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tree.rollout(rollouts)
        child = tree.choose()                                        # the most visited child is the new root
        ms.append((time.perf_counter() - t0) * 1e3)
        played.append(int(child.last_move))
    tree.close()
    return {"moves": played, "rollouts": rollouts, "playouts": playouts, "ms_per_move": float(np.mean(ms)), "ms_each": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fit-games", type=int, default=4096)
    ap.add_argument("--fit-seed", type=int, default=101)
    ap.add_argument("--quality-games", type=int, default=4096)
    ap.add_argument("--quality-seed", type=int, default=202)
    ap.add_argument("--genmoves", type=int, default=4, help="0: not measured")
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "amaf_prior_bench.json"))
    args = ap.parse_args()
    eng = reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0,
                                  min(max(args.fit_games, args.quality_games, 1), 4096))
    try:
        table, fit = fit_table(eng, args.fit_games, args.fit_seed)
        pos, played = positions_at_ply(eng, args.quality_games, args.quality_seed)
    finally:
        eng.close()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "fit": fit, "time": {}}
    starts = {"empty_board": torch.from_numpy(reinforce.initial_positions(args.records)).cuda(),
              "ply_40": pos[:args.records].contiguous()}
    for name, recs in starts.items():
        out["time"][name] = r = bench_time(recs, args.playouts, args.reps, args.seed)
        print(f"{name}: {r['records']} x {r['playouts']}: amaf {r['amaf_seconds'] * 1e3:.1f} ms, value "
              f"{r['value_seconds'] * 1e3:.1f} ms, x{r['ratio']:.3f}; the reduction alone {r['reduction_ms']:.3f} ms", flush=True)
    out["quality"] = q = bench_quality(pos, played, args.playouts, args.seed, table)
    print(f"quality at ply {q['ply']} ({q['positions']} positions, N={q['playouts']}): top-1 / top-5 "
          + ", ".join(f"{k} {q[k]['top1']:.4f} / {q[k]['top5']:.4f}" for k in ("uniform_playouts", "pattern_playouts",
                                                                              "uniform_prior")), flush=True)
    out["genmove"] = (bench_genmove(args.genmoves, args.rollouts, args.playouts, args.seed) if args.genmoves > 0
                      else "not measured")
    if args.genmoves > 0:
        print(f"net-free genmove: {out['genmove']['ms_per_move']:.0f} ms/move at {args.rollouts} rollouts", flush=True)
    out["match"] = "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

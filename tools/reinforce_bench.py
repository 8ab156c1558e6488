"""Rate of one REINFORCE iteration (bokego_amd/reinforce.py) on one MI355X: playout games/s and update positions/s.

    python tools/reinforce_bench.py [--games 256 4096] [--workers 16] [--reps 3] [--out profiles/reinforce_bench.json]
    python tools/reinforce_bench.py --one 4096     # warm-up, then ONE iteration at 4096 games (for rocprofv3)
    python tools/reinforce_bench.py --precision bf16 [...]   # the update's trunk convolutions on bf16 operands

An iteration is what reinforce.run_epoch does once: --workers batches of games/workers games each played in lock-step
between two fp32 engines (policy_19 against itself), then one AdamW step per batch.  Times are wall clock between device
synchronisations, the best of --reps after one warm-up iteration.
  playout          play_games as the learner runs it (no synchronisation inside the ply loop)
  breakdown        a second playout with a synchronisation after each phase of every ply: 'host' (bk_features_batch_u8,
                   staging, playing the moves, bookkeeping), 'engine' (upload + both LeafEngine.eval_device calls),
                   'sampler' (bkt_sample_moves + the 4-byte-per-game copy back)
  update           reinforce.update: positions/s = learner rows / seconds
The yardstick is the per-game path the reference's structure implies: selfplay.policy_self_play with HipPolicyNet
(one batch-1 forward per move, a second one when the sample is illegal) on --yardstick-games games.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bokego_amd import nnet, reinforce, selfplay, train  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")


def _sync():
    torch.cuda.synchronize()


def _iteration(net, opt, eng, opp, W, b, seed, it, timing=None):
    _sync()
    t0 = time.perf_counter()
    games = reinforce.play_games(eng, opp, W, b, seed, iteration=it, timing=timing)
    _sync()
    t1 = time.perf_counter()
    reinforce.update(net, opt, games, W, b)
    eng.set_weights(reinforce.engine_weights(net))
    _sync()
    t2 = time.perf_counter()
    return games, t1 - t0, t2 - t1


def bench_config(sd, games, workers, reps, seed=1, precision="fp32"):
    b = games // workers
    net = train.TrainablePolicyNet.from_state_dict(sd, precision=precision).eval()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-5)
    eng, opp = reinforce.policy_engine(sd, 0, games), reinforce.policy_engine(sd, 0, games)
    try:
        _iteration(net, opt, eng, opp, workers, b, seed, 0)                     # warm-up
        best_play, best_upd, rows, plies = float("inf"), float("inf"), 0, 0
        for r in range(reps):
            g, tp, tu = _iteration(net, opt, eng, opp, workers, b, seed, 1 + r)
            if tp < best_play:
                best_play, plies = tp, int(g.length.max())
            if tu < best_upd:
                best_upd, rows = tu, len(g.row_game)
        split = None
        for r in range(reps):
            timing = {}
            _sync()
            t0 = time.perf_counter()
            reinforce.play_games(eng, opp, workers, b, seed, iteration=100 + r, timing=timing)
            _sync()
            timing["total"] = time.perf_counter() - t0
            if split is None or timing["total"] < split["total"]:
                split = timing
    finally:
        eng.close()
        opp.close()
    return {"games": games, "workers": workers, "batch": b, "plies": plies,
            "playout_s": best_play, "playout_games_per_s": games / best_play,
            "breakdown_s": {k: split[k] for k in ("host", "engine", "sampler", "total")},
            "breakdown_share": {k: split[k] / split["total"] for k in ("host", "engine", "sampler")},
            "update_s": best_upd, "update_rows": rows, "update_positions_per_s": rows / best_upd,
            "iteration_games_per_s": games / (best_play + best_upd)}


def yardstick(sd, n_games):
    pi1, pi2 = nnet.HipPolicyNet(sd), nnet.HipPolicyNet(sd)
    torch.manual_seed(0)
    selfplay.policy_self_play(pi1, pi2, 2)                                       # warm-up
    t0 = time.perf_counter()
    games, _ = selfplay.policy_self_play(pi1, pi2, n_games)
    dt = time.perf_counter() - t0
    return {"path": "selfplay.policy_self_play + HipPolicyNet (batch 1 per move)", "games": n_games,
            "moves": sum(len(g) for g in games), "seconds": dt, "games_per_s": n_games / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yardstick-games", type=int, default=64)
    ap.add_argument("--one", type=int, default=None, help="warm up, then one iteration at this many games")
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32",
                    help="of the update's trunk convolutions (the playouts stay on the fp32 engines)")
    args = ap.parse_args()
    sd = train.load_weights(os.path.join(GOLDEN, "policy_19.bkw"))
    if args.one:
        b = args.one // args.workers
        net = train.TrainablePolicyNet.from_state_dict(sd, precision=args.precision).eval()
        opt = torch.optim.AdamW(net.parameters(), lr=1e-5)
        eng, opp = reinforce.policy_engine(sd, 0, args.one), reinforce.policy_engine(sd, 0, args.one)
        try:
            _iteration(net, opt, eng, opp, args.workers, b, 1, 0)
            g, tp, tu = _iteration(net, opt, eng, opp, args.workers, b, 1, 1)
        finally:
            eng.close()
            opp.close()
        print(json.dumps({"one": args.one, "playout_s": tp, "update_s": tu, "rows": len(g.row_game)}))
        return
    out = {"device": torch.cuda.get_device_name(0),
           "configs": [bench_config(sd, n, args.workers, args.reps, precision=args.precision) for n in args.games]}
    if args.precision != "fp32":
        out["update_precision"] = args.precision
    out["yardstick"] = yardstick(sd, args.yardstick_games)
    for c in out["configs"]:
        c["playout_speedup_vs_yardstick"] = c["playout_games_per_s"] / out["yardstick"]["games_per_s"]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

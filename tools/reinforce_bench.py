"""Rate of one REINFORCE iteration (bokego_amd/reinforce.py) on one MI355X: playout games/s and update positions/s.

    python tools/reinforce_bench.py [--games 256 4096] [--workers 16] [--reps 3] [--out profiles/reinforce_bench.json]
    python tools/reinforce_bench.py --rules both --out profiles/reinforce_device_rules_bench.json
    python tools/reinforce_bench.py --one 4096     # warm-up, then ONE iteration at 4096 games (for rocprofv3)
    python tools/reinforce_bench.py --precision bf16 [...]   # the update's trunk convolutions on bf16 operands

--rules device (the default, what the learner runs) or host picks play_games' rules.  --rules both compares them in one
process: per game count both paths are warmed up, then alternated --reps times, the best playout of each is kept, and
the file gets the seconds, games/s and phase split of each path, their ratio, the floor the ratio is held against
(FLOORS) and a meets_floor flag; then the update is timed in fp32 and bf16 on the device path's games, which gives the
whole iteration on either path.

An iteration is what reinforce.run_epoch does once: --workers batches of games/workers games each played in lock-step
between two fp32 engines (policy_19 against itself), then one AdamW step per batch.  Times are wall clock between device
synchronisations, the best of --reps after one warm-up iteration.
  playout          play_games as the learner runs it (no synchronisation inside the ply loop)
  breakdown        a second playout with a synchronisation after each phase of every ply.  Device rules: 'engine' (both
                   LeafEngine.eval_device calls), 'sampler' (bkt_sample_moves + the move history), 'rules' (the copy of
                   the learner's rows + bkt_play_moves), 'score' (bkt_area_score), 'download'.  Host rules: 'host'
                   (bk_features_batch_u8, staging, playing the moves, bookkeeping, scoring), 'engine' (upload + both
                   evaluations), 'sampler' (bkt_sample_moves + the 4-byte-per-game copy back)
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


FLOORS = {4096: 1.5, 256: 1.3}     # device-rules playout / host-rules playout, from the host loop's share


def _iteration(net, opt, eng, opp, W, b, seed, it, timing=None, rules="device"):
    _sync()
    t0 = time.perf_counter()
    games = reinforce.play_games(eng, opp, W, b, seed, iteration=it, timing=timing, rules=rules)
    _sync()
    t1 = time.perf_counter()
    reinforce.update(net, opt, games, W, b)
    eng.set_weights(reinforce.engine_weights(net))
    _sync()
    t2 = time.perf_counter()
    return games, t1 - t0, t2 - t1


def _split(eng, opp, workers, b, seed, reps, rules):
    """The phase split of the best of `reps` playouts with a synchronisation after each phase."""
    split = None
    for r in range(reps):
        timing = {}
        _sync()
        t0 = time.perf_counter()
        reinforce.play_games(eng, opp, workers, b, seed, iteration=100 + r, timing=timing, rules=rules)
        _sync()
        timing["total"] = time.perf_counter() - t0
        if split is None or timing["total"] < split["total"]:
            split = timing
    return {"seconds": split, "share": {k: v / split["total"] for k, v in split.items() if k != "total"}}


def _play(eng, opp, W, b, seed, it, rules):
    _sync()
    t0 = time.perf_counter()
    games = reinforce.play_games(eng, opp, W, b, seed, iteration=it, rules=rules)
    _sync()
    return games, time.perf_counter() - t0


def bench_both(sd, games, workers, reps, seed=1):
    """Host and device rules alternated in one process; then the update in fp32 and bf16 on the device path's games."""
    b = games // workers
    eng, opp = reinforce.policy_engine(sd, 0, games), reinforce.policy_engine(sd, 0, games)
    out = {"games": games, "workers": workers, "batch": b}
    try:
        for rules in ("device", "host"):
            _play(eng, opp, workers, b, seed, 0, rules)                          # warm-up
        best = {"device": float("inf"), "host": float("inf")}
        for r in range(reps):
            for rules in ("device", "host"):
                g, dt = _play(eng, opp, workers, b, seed, 1 + r, rules)
                best[rules] = min(best[rules], dt)
        for rules in ("device", "host"):
            out[rules] = {"playout_s": best[rules], "playout_games_per_s": games / best[rules],
                          "breakdown": _split(eng, opp, workers, b, seed, reps, rules)}
        out["device_speedup"] = best["host"] / best["device"]
        if games in FLOORS:
            out["floor"] = FLOORS[games]
            out["meets_floor"] = bool(out["device_speedup"] >= FLOORS[games])
        out["update"] = {}
        for precision in ("fp32", "bf16"):
            net = train.TrainablePolicyNet.from_state_dict(sd, precision=precision).eval()
            opt = torch.optim.AdamW(net.parameters(), lr=1e-5)
            upd = float("inf")
            for r in range(reps + 1):                                            # the first one warms up
                _sync()
                t0 = time.perf_counter()
                reinforce.update(net, opt, g, workers, b)
                _sync()
                if r:
                    upd = min(upd, time.perf_counter() - t0)
            out["update"][precision] = {"update_s": upd, "rows": len(g.row_game),
                                        "iteration_s": {k: best[k] + upd for k in best},
                                        "iteration_games_per_s": {k: games / (best[k] + upd) for k in best}}
            del net, opt
    finally:
        eng.close()
        opp.close()
    return out


def bench_config(sd, games, workers, reps, seed=1, precision="fp32", rules="device"):
    b = games // workers
    net = train.TrainablePolicyNet.from_state_dict(sd, precision=precision).eval()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-5)
    eng, opp = reinforce.policy_engine(sd, 0, games), reinforce.policy_engine(sd, 0, games)
    try:
        _iteration(net, opt, eng, opp, workers, b, seed, 0, rules=rules)        # warm-up
        best_play, best_upd, rows, plies = float("inf"), float("inf"), 0, 0
        for r in range(reps):
            g, tp, tu = _iteration(net, opt, eng, opp, workers, b, seed, 1 + r, rules=rules)
            if tp < best_play:
                best_play, plies = tp, int(g.length.max())
            if tu < best_upd:
                best_upd, rows = tu, len(g.row_game)
        split = _split(eng, opp, workers, b, seed, reps, rules)
    finally:
        eng.close()
        opp.close()
    return {"games": games, "workers": workers, "batch": b, "plies": plies, "rules": rules,
            "playout_s": best_play, "playout_games_per_s": games / best_play,
            "breakdown_s": split["seconds"], "breakdown_share": split["share"],
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
    ap.add_argument("--rules", choices=["host", "device", "both"], default="device",
                    help="play_games' rules; both: the two paths alternated in one process, their ratio and the floors")
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
            rules = "device" if args.rules == "both" else args.rules
            _iteration(net, opt, eng, opp, args.workers, b, 1, 0, rules=rules)
            g, tp, tu = _iteration(net, opt, eng, opp, args.workers, b, 1, 1, rules=rules)
        finally:
            eng.close()
            opp.close()
        print(json.dumps({"one": args.one, "rules": rules, "playout_s": tp, "update_s": tu, "rows": len(g.row_game)}))
        return
    if args.rules == "both":
        out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
               "configs": [bench_both(sd, n, args.workers, args.reps) for n in args.games]}
    else:
        out = {"device": torch.cuda.get_device_name(0),
               "configs": [bench_config(sd, n, args.workers, args.reps, precision=args.precision, rules=args.rules)
                           for n in args.games]}
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

"""What ownership and criticality from the playouts (bkt_owner_counts) cost and whether the criticality term of the
prior wins games, on one MI355X.  By tools/rave_bench.py's protocol: a warm-up, the paths alternated in one process, best of
--reps.  One gate: the fused kernel is no slower than the composition it replaces; everything else is recorded.

    python tools/ownership_bench.py kernel    [--records 1024] [--playouts 64] [--reps 3]
    python tools/ownership_bench.py ownership [--records 1024] [--playouts 64] [--reps 3]
    python tools/ownership_bench.py genmove   [--genmoves 8] [--rollouts 400] [--playouts 64] [--gamma 1] [--reps 3]
    python tools/ownership_bench.py quality   [--games 4096] [--playouts 64]
    python tools/ownership_bench.py match --gamma G [--games 100] [--rollouts 400] [--playouts 64] [--rave 4] [--opening-plies 4]
    python tools/ownership_bench.py all       # every part above, the match for gamma 0.5, 1 and 2, each a child process
                                              # under its own time limit (--limit seconds)
    (each with [--out profiles/ownership_bench.json]: a part replaces its own entry of that file and leaves the others;
     genmove and match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

kernel      bkt_owner_counts against what could be done before it on the same --records x --playouts final records:
            bkt_area_score(owner=True) and torch's reductions -- owner.view(R, n, 81) summed three ways and the score compared
            (no margin histogram: the composition does less).  From the empty board and from ply 40 of policy_19 games, by HIP
            events, alternated, best of --reps; `ratio` = composition / fused, and the gate is ratio >= 1.
ownership   rollout.playout_ownership against rollout.playout_value end to end on the same records, uploads and downloads
            included (wall clock around a synchronised call); `ratio` = ownership / value.
genmove     ms per move of --genmoves moves of a net-free search from the empty board, --rollouts rollouts a move, with
            playout_criticality=--gamma and without it: two trees alternated move by move, best mean of --reps runs.
quality     at ply 40 of --games policy_19 games, how often the policy's move is the top-1 / among the top-5 of the prior for
            gamma in 0, 0.5, 1, 2 (gamma = 0 is tools/amaf_prior_bench.py's figure).
match       --games games, colours alternated, --rollouts rollouts a move: `gtp --playout-value N --playout-prior 1
            --playout-rave K --playout-criticality G` against the same engine without --playout-criticality; each
            colour-swapped pair starts from --opening-plies seeded random moves.  A result within 40..60 is "no difference shown".
A part that did not run reads "not measured".
"""
import argparse
import json
import os
import subprocess
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
PARTS = ("kernel", "ownership", "genmove", "quality", "match", "all")
GAMMAS = (0.5, 1.0, 2.0)


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _ply_40(games):
    from amaf_prior_bench import positions_at_ply
    from bokego_amd.train import load_weights
    eng = reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 4096)
    try:
        return positions_at_ply(eng, games, 202)
    finally:
        eng.close()


def _starts(records):
    return {"empty_board": torch.from_numpy(reinforce.initial_positions(records)).cuda(),
            "ply_40": _ply_40(4096)[0][:records].contiguous()}


def composed(pos, records, playouts, komi):
    """bkt_owner_counts' black, white, agree and black_wins the way the parent commit can: the owner array and torch."""
    score, owner = rollout._area_score_device(pos, komi, True)
    o = owner.view(records, playouts, 81)
    bw = (score > 0).view(records, playouts, 1)
    isb, isw = o == 1, o == -1
    return (isb.sum(1, dtype=torch.int32), isw.sum(1, dtype=torch.int32),
            ((isb & bw) | (isw & ~bw)).sum(1, dtype=torch.int32), bw.sum((1, 2), dtype=torch.int32))


def bench_kernel(recs, playouts, reps, seed):
    pos = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", final=True).final
    R = len(recs)
    paths = {"fused": lambda: T.owner_counts(pos, R, playouts, L.KOMI), "composed": lambda: composed(pos, R, playouts, L.KOMI)}
    f, c = paths["fused"](), paths["composed"]()                       # warm-up, and the same integers
    assert all(torch.equal(x, y) for x, y in zip((f[0], f[1], f[2], f[4]), c))
    best = {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            ms = _event_ms(fn)
            best[name] = min(ms, best.get(name, ms))
    return {"records": R, "playouts": playouts, "rows": R * playouts, "owner_array_bytes": R * playouts * 81,
            "fused_ms": best["fused"], "composed_ms": best["composed"], "ratio": best["composed"] / best["fused"],
            "gate_ratio_at_least_1": bool(best["composed"] / best["fused"] >= 1.0)}


def part_kernel(args):
    out = {}
    for name, recs in _starts(args.records).items():
        out[name] = r = bench_kernel(recs, args.playouts, args.reps, args.seed)
        print(f"{name}: {r['records']} x {r['playouts']}: fused {r['fused_ms']:.3f} ms, area score + torch {r['composed_ms']:.3f} ms, "
              f"x{r['ratio']:.3f} ({'gate met' if r['gate_ratio_at_least_1'] else 'GATE MISSED'})", flush=True)
    return out


def part_ownership(args):
    out = {}
    for name, recs in _starts(args.records).items():
        recs = recs.cpu().numpy()                                    # uploads included
        paths = {"ownership": lambda: rollout.playout_ownership(recs, args.playouts, args.seed),
                 "value": lambda: rollout.playout_value(recs, args.playouts, args.seed)}
        for fn in paths.values():                                    # warm-up
            fn()
        best, last = {}, {}
        for _ in range(args.reps):                                   # alternated
            for k, fn in paths.items():
                last[k], dt = _timed(fn)
                best[k] = min(dt, best.get(k, dt))
        assert np.array_equal(last["ownership"].value, last["value"])
        out[name] = r = {"records": len(recs), "playouts": args.playouts, "ownership_seconds": best["ownership"],
                         "value_seconds": best["value"], "ratio": best["ownership"] / best["value"]}
        print(f"{name}: playout_ownership {r['ownership_seconds'] * 1e3:.2f} ms, playout_value {r['value_seconds'] * 1e3:.2f} ms, "
              f"x{r['ratio']:.3f}", flush=True)
    return out


def part_genmove(args):
    kinds = {"criticality": {"playout_criticality": args.gamma}, "plain": {}}
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
    out = {"rollouts": args.rollouts, "playouts": args.playouts, "playout_criticality": args.gamma, "genmoves": args.genmoves,
           "criticality": best["criticality"], "plain": best["plain"],
           "ratio": best["criticality"]["ms_per_move"] / best["plain"]["ms_per_move"]}
    print(f"net-free genmove at {args.rollouts} rollouts: with playout_criticality={args.gamma:g} "
          f"{out['criticality']['ms_per_move']:.2f} ms/move, without {out['plain']['ms_per_move']:.2f}, x{out['ratio']:.3f}", flush=True)
    return out


def part_quality(args):
    pos, played = _ply_40(args.games)
    recs = pos.cpu().numpy()
    amaf = rollout.playout_amaf(pos, args.playouts, args.seed)
    own = rollout.playout_ownership(pos, args.playouts, args.seed)
    assert np.array_equal(amaf.value, own.value)                     # the same games
    crit = own.criticality()
    rows = np.arange(len(recs))
    out = {"ply": 40, "positions": int(len(recs)), "playouts": args.playouts,
           "mean_abs_criticality": float(np.abs(crit).mean()), "max_criticality_mean": float(crit.max(1).mean())}
    for gamma in (0.0,) + GAMMAS:
        prior = rollout.amaf_prior(recs, amaf, criticality=crit, gamma=gamma)
        order = np.argsort(-prior, 1, kind="stable")
        out[f"gamma={gamma:g}"] = r = {"top1": float((order[:, 0] == played).mean()),
                                       "top5": float((order[:, :5] == played[:, None]).any(1).mean()),
                                       "mean_prior_of_the_move": float(prior[rows, played].mean())}
        print(f"gamma {gamma:g}: top-1 {100 * r['top1']:.1f} %, top-5 {100 * r['top5']:.1f} % over {len(recs)} positions", flush=True)
    return out


def part_match(args):
    from bokego_amd.gtp import NativeGTP

    def engine(name, **more):
        return match.InProcessEngine(NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=args.rollouts,
                                               playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                                               playout_rules=args.rules, **more), name=name)

    a, b = engine("criticality", playout_criticality=args.gamma), engine("plain")
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["criticality_wins"]
    share = 100.0 * wins / args.games
    res.update(playout_criticality=args.gamma, playout_rave=args.rave, rollouts=args.rollouts, playouts=args.playouts,
               opening_plies=args.opening_plies, seed=args.seed,
               verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("criticality wins beyond the margin" if share > 60.0 else "criticality loses beyond the margin"))
    print(f"match gamma={args.gamma:g}: criticality {wins} : {res['plain_wins']} plain over {args.games} games -- {res['verdict']}; "
          f"ms/move {res['ms_per_move']['criticality']:.2f} / {res['ms_per_move']['plain']:.2f}", flush=True)
    a.close()
    b.close()
    return res


def part_all(args, argv):
    """Every part a child process under its own time limit; the first that fails or runs out of time ends the run."""
    common = [a for a in argv if a != "all"]
    jobs = [["kernel"], ["ownership"], ["genmove"], ["quality"]] + [["match", "--gamma", f"{g:g}"] for g in GAMMAS]
    for job in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), job[0]] + common + job[1:]
        print("+", " ".join(job), flush=True)
        rc = subprocess.run(cmd, timeout=args.limit).returncode
        if rc != 0:
            sys.exit(f"{' '.join(job)} ended with status {rc}: nothing more is started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--genmoves", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--gamma", type=float, default=1.0, metavar="G")
    ap.add_argument("--rave", type=float, default=4.0, metavar="K")
    ap.add_argument("--games", type=int, default=None, help="match: games (100); quality: policy games (4096)")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--rules", choices=("device", "host"), default="device")
    ap.add_argument("--limit", type=float, default=240.0, help="all: seconds each child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ownership_bench.json"))
    args = ap.parse_args()
    if args.part == "all":
        return part_all(args, sys.argv[1:])
    if args.games is None:
        args.games = 100 if args.part == "match" else 4096
    out = {"kernel": "not measured", "ownership": "not measured", "genmove": "not measured", "quality": "not measured",
           "match": {f"gamma={g:g}": "not measured" for g in GAMMAS}}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0) if args.rules == "device" else "none (host rules: a dry run)"
    if args.part == "match":
        key = f"gamma={args.gamma:g}" + ("" if args.seed == ap.get_default("seed") else f",seed={args.seed}")
        out["match"][key] = part_match(args)
    else:
        out[args.part] = {"kernel": part_kernel, "ownership": part_ownership, "genmove": part_genmove,
                          "quality": part_quality}[args.part](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""What the move weights of a position in one launch (bkt_move_weights) cost, what the pattern term of the prior
knows and whether it wins games, on one MI355X.  One figure has a threshold, the gate; the others are recorded.  By
tools/rave_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps.

    python tools/pattern_prior_bench.py gate    [--records 1024] [--reps 3]
    python tools/pattern_prior_bench.py predict [--quality-games 4096] [--playouts 64]
    python tools/pattern_prior_bench.py genmove [--genmoves 8] [--rollouts 400] [--playouts 64] [--mu 1] [--reps 3]
    python tools/pattern_prior_bench.py match --mu MU [--games 100] [--rollouts 400] [--playouts 64] [--opening-plies 4] [--seed 1]
    (each with [--out profiles/pattern_prior_bench.json]: a part replaces its own entry of that file and leaves the others;
     genmove and match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

No table ships: every part fits its own as tools/tactical_playout_bench.py does, patterns.fit's and tactics.fit's counts on
--fit-games policy_19 games with seed --fit-seed -- other games than the ones evaluated (--quality-seed).

gate        bkt_move_weights on --records records against the composition it replaces on the same records: bkt_pattern_codes,
            bkt_tactical_codes, bkt_playout_step with BKT_MOVE_NONE on a copy, and torch's gathers, product, shift and max,
            by HIP events, alternated, best of --reps, from the empty board and from ply 40 of policy_19 games.  `ratio` =
            composition / fused must be >= 1.0: a fused launch slower than the launches it replaces has no reason to exist.
predict     DESIGN 19's measurement: at ply 40 of --quality-games policy_19 games, the share of positions in which the move the
            policy played is the top-1, and among the top-5, of rollout.pattern_prior alone (patterns, tactics, both) and of
            amaf_prior(playout_amaf(N = --playouts, uniform playouts), weights of both tables, mu) for mu in 0, 0.5, 1, 2.
genmove     ms per move of --genmoves moves of a net-free search from the empty board, --rollouts rollouts a move, with
            playout_pattern_prior=--mu and without: two trees alternated move by move, the whole run --reps times, best mean.
match       --games games, colours alternated, --rollouts rollouts a move: the in-process GTP engine of `gtp --playout-value N
            --playout-prior 1 --playout-rave 4 --playout-pattern-prior MU` (the fitted tables as --prior-patterns and
            --prior-tactics; uniform playouts) against the same engine without the flag, tools/rave_bench.py's protocol: pairs
            of games from --opening-plies seeded random moves.  A result within 40..60 is "no difference shown".
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
PARTS = ("gate", "predict", "genmove", "match")
MUS = (0.5, 1.0, 2.0)
GATE_RATIO = 1.0


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fitted(args, positions=False):
    """The fitted tables, and with positions=True the ply-40 records and the moves played there."""
    from amaf_prior_bench import positions_at_ply
    from bokego_amd.train import load_weights
    from tactical_playout_bench import fit_tables
    eng = reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 4096)
    try:
        tabs = fit_tables(eng, args.fit_games, args.fit_seed)
        pos, played = positions_at_ply(eng, args.quality_games, args.quality_seed) if positions else (None, None)
    finally:
        eng.close()
    return tabs, pos, played


def composition(recs, table, tactics):
    """What the parent commit can do: three launches and torch.  table, tactics: int64 [entries] on the device."""
    idx = T.pattern_codes(recs).to(torch.int64)
    code = T.tactical_codes(recs).to(torch.int64)
    scratch = recs.clone()
    playable = torch.empty((len(recs), 81), dtype=torch.uint8, device=recs.device)
    T.playout_step(scratch, torch.full((len(recs),), T.MOVE_NONE, dtype=torch.int32, device=recs.device), None, None, playable)
    w = ((table[idx].clamp_(min=1) * tactics[code]) >> 8).clamp_(min=1)
    return (w * (playable != 0)).to(torch.int32)


def bench_gate(recs, tabs, reps):
    pat, tac = tabs["patterns"].device(recs.device), tabs["tactics"].device(recs.device)
    pat64, tac64 = pat.to(torch.int64) & 0xFFFF, tac.to(torch.int64) & 0xFFFF     # made once, outside the timing
    paths = {"fused": lambda: T.move_weights(recs, pat, tac), "composition": lambda: composition(recs, pat64, tac64)}
    assert torch.equal(paths["fused"](), paths["composition"]())      # warm-up, and the same integers
    best = {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            ms = _event_ms(fn)
            best[name] = min(ms, best.get(name, ms))
    ratio = best["composition"] / best["fused"]
    return {"records": len(recs), "fused_ms": best["fused"], "composition_ms": best["composition"], "ratio": ratio,
            "gate": GATE_RATIO, "passes": bool(ratio >= GATE_RATIO)}


def part_gate(args):
    tabs, pos, _ = fitted(args, positions=True)
    starts = {"empty_board": torch.from_numpy(reinforce.initial_positions(args.records)).cuda(),
              "ply_40": pos[:args.records].contiguous()}
    out = {}
    for name, recs in starts.items():
        out[name] = r = bench_gate(recs, tabs, args.reps)
        print(f"{name}: {r['records']} records: fused {r['fused_ms']:.4f} ms, composition {r['composition_ms']:.4f} ms, "
              f"x{r['ratio']:.2f} ({'passes' if r['passes'] else 'FAILS'} the gate of {GATE_RATIO})", flush=True)
    return out


def _top(prior, played):
    order = np.argsort(-prior, 1, kind="stable")
    return {"top1": float((order[:, 0] == played).mean()), "top5": float((order[:, :5] == played[:, None]).any(1).mean()),
            "mean_prior_of_the_move": float(prior[np.arange(len(prior)), played].mean())}


def part_predict(args):
    tabs, pos, played = fitted(args, positions=True)
    recs = pos.cpu().numpy()
    n_legal = rollout.legal_host(recs).sum(1)
    out = {"ply": 40, "positions": int(len(recs)), "playouts": args.playouts, "value_seed": args.seed,
           "fit": {"games": args.fit_games, "seed": args.fit_seed}, "quality_seed": args.quality_seed,
           "uniform_prior": {"top1": float((1.0 / n_legal).mean()), "top5": float((np.minimum(5, n_legal) / n_legal).mean())},
           "pattern_prior": {}, "amaf_prior": {}}
    for name, (p, t) in (("patterns", (tabs["patterns"], None)), ("tactics", (None, tabs["tactics_alone"])),
                         ("both", (tabs["patterns"], tabs["tactics"]))):
        out["pattern_prior"][name] = _top(rollout.pattern_prior(recs, rollout.move_weights(pos, p, t)), played)
    amaf = rollout.playout_amaf(pos, args.playouts, args.seed)        # uniform playouts: DESIGN 19's 7.8 % and 21.4 % at mu = 0
    w = rollout.move_weights(pos, tabs["patterns"], tabs["tactics"])
    for mu in (0.0,) + MUS:
        out["amaf_prior"][f"mu={mu:g}"] = _top(rollout.amaf_prior(recs, amaf, weights=w, mu=mu), played)
    for kind in ("pattern_prior", "amaf_prior"):
        print(f"{kind} at ply 40 ({len(recs)} positions): top-1 / top-5 "
              + ", ".join(f"{k} {v['top1']:.4f} / {v['top5']:.4f}" for k, v in out[kind].items()), flush=True)
    return out


def _prior_kw(args, tabs, mu):
    return dict(playout_pattern_prior=mu, prior_patterns=tabs["patterns"], prior_tactics=tabs["tactics"])


def part_genmove(args, tabs):
    kinds = {"pattern_prior": _prior_kw(args, tabs, args.mu), "plain": {}}
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
    out = {"rollouts": args.rollouts, "playouts": args.playouts, "mu": args.mu, "genmoves": args.genmoves,
           "pattern_prior": best["pattern_prior"], "plain": best["plain"],
           "ratio": best["pattern_prior"]["ms_per_move"] / best["plain"]["ms_per_move"]}
    print(f"net-free genmove at {args.rollouts} rollouts: with playout_pattern_prior={args.mu:g} "
          f"{out['pattern_prior']['ms_per_move']:.2f} ms/move, without {out['plain']['ms_per_move']:.2f}, x{out['ratio']:.3f}",
          flush=True)
    return out


def part_match(args, tabs):
    from bokego_amd.gtp import NativeGTP

    def engine(name, **more):
        return match.InProcessEngine(NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=args.rollouts,
                                               playout_value=args.playouts, playout_prior=1.0, playout_rave=4.0,
                                               playout_rules=args.rules, **more), name=name)

    a, b = engine("pattern", **_prior_kw(args, tabs, args.mu)), engine("plain")
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["pattern_wins"]
    share = 100.0 * wins / args.games
    res.update(mu=args.mu, playout_rave=4.0, rollouts=args.rollouts, playouts=args.playouts, opening_plies=args.opening_plies,
               seed=args.seed, verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("the pattern prior wins beyond the margin" if share > 60.0 else "the pattern prior loses beyond the margin"))
    print(f"match mu={args.mu:g}: pattern prior {wins} : {res['plain_wins']} plain over {args.games} games -- {res['verdict']}; "
          f"ms/move {res['ms_per_move']['pattern']:.2f} / {res['ms_per_move']['plain']:.2f}", flush=True)
    return res


def host_tables(args):
    """--rules host: tables fitted on the host mirror from a few uniformly random games (a dry run needs no policy net)."""
    from bokego_amd import patterns, tactics
    start = reinforce.initial_positions(8)
    fin = rollout.random_playouts(start, args.fit_seed, rules="host", max_plies=60)
    table = patterns.fit(start, fin.moves, rules="host")
    return {"patterns": table, "tactics": tactics.fit(start, fin.moves, table, rules="host")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fit-games", type=int, default=4096)
    ap.add_argument("--fit-seed", type=int, default=101)
    ap.add_argument("--quality-games", type=int, default=4096)
    ap.add_argument("--quality-seed", type=int, default=202)
    ap.add_argument("--genmoves", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--mu", type=float, default=1.0)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--rules", choices=("device", "host"), default="device")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pattern_prior_bench.json"))
    args = ap.parse_args()
    if args.rules == "host" and args.part in ("gate", "predict"):
        ap.error("gate and predict measure the device: no --rules host")
    out = {"gate": "not measured", "predict": "not measured", "genmove": "not measured",
           "match": {f"mu={mu:g}": "not measured" for mu in MUS}}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0) if args.rules == "device" else "none (host rules: a dry run)"
    if args.part in ("gate", "predict"):
        out[args.part] = (part_gate if args.part == "gate" else part_predict)(args)
    else:
        tabs = host_tables(args) if args.rules == "host" else fitted(args)[0]
        if args.part == "match":
            key = f"mu={args.mu:g}" + ("" if args.seed == ap.get_default("seed") else f",seed={args.seed}")
            out["match"][key] = part_match(args, tabs)
        else:
            out["genmove"] = part_genmove(args, tabs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""What the last-good-reply playouts and their table's update (bkt_reply_playouts, bkt_reply_update) cost and whether
they win games, on one MI355X.  Nothing here has a threshold except the match's 40..60 band: the figures are recorded.  By
tools/rave_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps.

    python tools/reply_playout_bench.py playouts [--games 4096 65536] [--reps 3]
    python tools/reply_playout_bench.py update   [--records 1024] [--playouts 64] [--reps 3]
    python tools/reply_playout_bench.py genmove  [--genmoves 8] [--rollouts 400] [--playouts 64] [--rave 4] [--reps 3]
    python tools/reply_playout_bench.py match    [--games 100] [--rollouts 400] [--playouts 64] [--opening-plies 4] [--seed 1]
    (each with [--out profiles/reply_playout_bench.json]: a part replaces its own entry of that file and leaves the others;
     genmove and match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

playouts    bkt_reply_playouts against bkt_tactical_playouts (the kernel of the commit before: it is unchanged) with the same
            fitted pattern and tactics tables, --games games from the empty board, by HIP events, alternated, best of --reps:
            first with the all-255 table (the wrapper alone), then with a table learned from one batch.  Time ratios and
            mean game lengths.
update      bkt_reply_update against bkt_amaf_counts_sides on the same --records x --playouts histories (a scan of the
            same bytes), from the empty board and from ply 40 of policy_19 games.
genmove     ms per move of --genmoves moves of a net-free search (playout_prior=1, playout_rave=--rave) from the empty board,
            --rollouts rollouts a move, with playout_replies and without: two trees alternated move by move, the whole run
            --reps times, best mean.  One more tree, not timed, counts the plies the table decided (from each request's
            history and the table before it) and the table's occupancy after every move.
match       --games games, colours alternated, --rollouts rollouts a move: `gtp --playout-value N --playout-prior 1
            --playout-rave K --playout-replies` against the same engine without --playout-replies, every pair of games from
            --opening-plies seeded random moves.  Wins and ms/move of both; a result within 40..60 is "no difference shown".
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
from bokego_amd import match, reinforce, replies, rollout  # noqa: E402
from bokego_amd.mcts_native import NativeMCTS, Position  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
PARTS = ("playouts", "update", "genmove", "match")


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _policy_engine():
    from bokego_amd.train import load_weights
    return reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, 4096)


def bench_playouts(games, reps, seed, pat, tac):
    dev = torch.device("cuda", 0)
    start = torch.from_numpy(reinforce.initial_positions(games)).to(dev)
    ctr = L.counters_to_device(rollout.default_counters(games, np.zeros(games, np.int32)), games, dev)
    w, t = pat.device(dev), tac.device(dev)
    empty = replies.ReplyTable.empty().device(dev)
    learned = replies.ReplyTable.empty().device(dev).clone()
    pos = start.clone()                                               # one batch, scored, folded into the table
    moves = T.reply_playouts(pos, seed, ctr, w, t, learned, rollout.MAX_PLIES)[2]
    won = ((T.area_score(pos, L.KOMI) > 0) == L.black_to_move(start)).to(torch.uint8)
    T.reply_update(start, moves, won, games, 1, learned)

    def run(play, *tables):
        return lambda: play(start.clone(), seed + 1, ctr, *tables, rollout.MAX_PLIES)[1]

    paths = {"tactical": run(T.tactical_playouts, w, t), "reply_empty": run(T.reply_playouts, w, t, empty),
             "reply_learned": run(T.reply_playouts, w, t, learned)}
    assert torch.equal(paths["tactical"](), paths["reply_empty"]())   # warm-up, and the same games
    paths["reply_learned"]()
    best, plies = {}, {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            ms, n = _event_ms(fn)
            best[name], plies[name] = min(ms, best.get(name, ms)), float(n.float().mean())
    return {"games": games, "occupancy_learned": int((learned <= 80).sum()),
            **{name: {"ms": best[name], "plies_mean": plies[name]} for name in paths},
            "ratio_empty": best["reply_empty"] / best["tactical"], "ratio_learned": best["reply_learned"] / best["tactical"]}


def part_playouts(args):
    from tactical_playout_bench import fit_tables
    eng = _policy_engine()
    try:
        tables = fit_tables(eng, 4096, 101)
    finally:
        eng.close()
    out = {}
    for games in args.games:
        out[str(games)] = r = bench_playouts(games, args.reps, args.seed, tables["patterns"], tables["tactics"])
        print(f"{games} games: tactical {r['tactical']['ms']:.2f} ms ({r['tactical']['plies_mean']:.1f} plies), all-255 table "
              f"x{r['ratio_empty']:.3f}, learned table x{r['ratio_learned']:.3f} ({r['reply_learned']['plies_mean']:.1f} plies)",
              flush=True)
    return out


def bench_update(recs, playouts, reps, seed):
    run = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", history=True)
    won, moves = run.won.to(torch.uint8).reshape(-1), run.moves
    table = replies.ReplyTable.empty().device(recs.device).clone()
    scratch = torch.empty((T.load().bkt_reply_scratch_bytes(len(recs)),), dtype=torch.uint8, device=recs.device)
    paths = {"reply_update": lambda: T.reply_update(recs, moves, won, len(recs), playouts, table, scratch),
             "amaf_sides": lambda: T.amaf_counts_sides(moves, won, len(recs), playouts)}
    for fn in paths.values():                                        # warm-up
        fn()
    best = {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            ms, _ = _event_ms(fn)
            best[name] = min(ms, best.get(name, ms))
    return {"records": len(recs), "playouts": playouts, "max_plies": int(moves.shape[1]), "history_bytes": int(moves.numel() * 2),
            "reply_update_ms": best["reply_update"], "amaf_sides_ms": best["amaf_sides"],
            "ratio": best["reply_update"] / best["amaf_sides"]}


def part_update(args):
    from amaf_prior_bench import positions_at_ply
    eng = _policy_engine()
    try:
        pos, _ = positions_at_ply(eng, 4096, 202)
    finally:
        eng.close()
    starts = {"empty_board": torch.from_numpy(reinforce.initial_positions(args.records)).cuda(),
              "ply_40": pos[:args.records].contiguous()}
    out = {}
    for name, recs in starts.items():
        out[name] = r = bench_update(recs, args.playouts, args.reps, args.seed)
        print(f"{name}: {r['records']} x {r['playouts']}: update {r['reply_update_ms']:.3f} ms, two-sided AMAF "
              f"{r['amaf_sides_ms']:.3f} ms, x{r['ratio']:.3f}", flush=True)
    return out


def _tree(args, **more):
    return NativeMCTS(Position(), None, None, playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                      playout_seed=args.seed, playout_rules=args.rules, **more)


def table_statistics(args):
    """One search with the option, not timed: per move, the plies its requests played, those the table decided, and the
    table's occupancy after the move."""
    t = _tree(args, playout_replies=True)
    ev, seen = t.evaluator, {"plies": 0, "decided": 0}
    submit = ev.submit

    def counting(recs, n_policy):
        before = ev.replies.copy()
        h = submit(recs, n_policy)
        moves = rollout._numpy(h.run.moves)
        seen["plies"] += int((np.cumsum(moves <= rollout.MOVE_NONE, 1) == 0).sum())
        seen["decided"] += replies.reply_plies_of(before, np.ascontiguousarray(recs, np.uint8), moves, ev.playouts)
        return h

    ev.submit = counting
    out = []
    for _ in range(args.genmoves):
        seen.update(plies=0, decided=0)
        t.rollout(args.rollouts)
        t.choose()
        out.append({"plies": seen["plies"], "reply_plies": seen["decided"], "share": seen["decided"] / max(seen["plies"], 1),
                    "occupancy": ev.replies.occupancy()})
    t.close()
    return out


def part_genmove(args):
    kinds = {"replies": {"playout_replies": True}, "plain": {}}
    best = {}
    for _ in range(args.reps):
        trees = {k: _tree(args, **kw) for k, kw in kinds.items()}
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
    per_move = table_statistics(args)
    plies, decided = sum(m["plies"] for m in per_move), sum(m["reply_plies"] for m in per_move)
    out = {"rollouts": args.rollouts, "playouts": args.playouts, "playout_rave": args.rave, "genmoves": args.genmoves,
           "replies": best["replies"], "plain": best["plain"],
           "ratio": best["replies"]["ms_per_move"] / best["plain"]["ms_per_move"],
           "table": {"per_move": per_move, "plies": plies, "reply_plies": decided, "share": decided / max(plies, 1)}}
    print(f"net-free genmove at {args.rollouts} rollouts: with playout_replies {out['replies']['ms_per_move']:.2f} ms/move, "
          f"without {out['plain']['ms_per_move']:.2f}, x{out['ratio']:.3f}; the table decided {100 * out['table']['share']:.1f} % "
          f"of {plies} plies, occupancy {[m['occupancy'] for m in per_move]}", flush=True)
    return out


def part_match(args):
    from bokego_amd.gtp import NativeGTP

    def engine(name, **more):
        return match.InProcessEngine(NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=args.rollouts,
                                               playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                                               playout_rules=args.rules, **more), name=name)

    a, b = engine("replies", playout_replies=True), engine("plain")
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["replies_wins"]
    share = 100.0 * wins / args.games
    res.update(playout_rave=args.rave, rollouts=args.rollouts, playouts=args.playouts, opening_plies=args.opening_plies,
               seed=args.seed, verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("replies win beyond the margin" if share > 60.0 else "replies lose beyond the margin"))
    print(f"match: replies {wins} : {res['plain_wins']} plain over {args.games} games -- {res['verdict']}; ms/move "
          f"{res['ms_per_move']['replies']:.2f} / {res['ms_per_move']['plain']:.2f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--games", type=int, nargs="+", default=None, help="playouts: the batch sizes (4096 65536); match: the games (100)")
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--genmoves", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--rave", type=float, default=4.0, metavar="K")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--rules", choices=("device", "host"), default="device")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reply_playout_bench.json"))
    args = ap.parse_args()
    if args.part == "match":
        args.games = 100 if args.games is None else args.games[0]
    elif args.games is None:
        args.games = [4096, 65536]
    out = {part: "not measured" for part in PARTS}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0) if args.rules == "device" else "none (host rules: a dry run)"
    out[args.part] = {"playouts": part_playouts, "update": part_update, "genmove": part_genmove, "match": part_match}[args.part](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

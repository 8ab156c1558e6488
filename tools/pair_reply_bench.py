"""What replies keyed by the last two moves (bkt_reply2_playouts, bkt_reply2_update) cost beside the single-move
table of DESIGN 24, and whether they win games, on one MI355X.  Nothing here has a threshold except the match's 40..60 band:
the figures are recorded.  tools/reply_playout_bench.py's protocol: a warm-up, the paths alternated in one process, best of
--reps by HIP events.

    python tools/pair_reply_bench.py playouts [--games 4096 65536] [--reps 3]
    python tools/pair_reply_bench.py update   [--shapes 1024x64 81x64] [--reps 3]
    python tools/pair_reply_bench.py genmove  [--genmoves 8] [--rollouts 400] [--playouts 64] [--rave 4] [--reps 3]
    python tools/pair_reply_bench.py match    [--games 100] [--rollouts 400] [--playouts 64] [--opening-plies 4] [--seed 1]
    (each with [--out profiles/pair_reply_bench.json]: a part replaces its own entry of that file and leaves the others;
     genmove and match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

playouts    bkt_reply2_playouts against bkt_reply_playouts (unchanged code) with the same fitted pattern and tactics tables,
            --games games from the empty board: first with all-255 pairs over an all-255 single table (what staging 13 KB and
            the second lookup cost), then each with its own table learned from one batch.  Time ratios, mean game lengths.
update      bkt_reply2_update against bkt_reply_update on the same records x playouts histories from the empty board.  It
            does strictly more than the old update does: 82 planes instead of one.
genmove     ms per move of a net-free search (playout_prior=1, playout_rave=--rave) from the empty board with
            playout_reply_pairs and with playout_replies: two trees alternated move by move, the whole run --reps times, best
            mean.  One more tree, not timed, counts the plies the pair entries and the single entries decided and the
            occupancy of both parts of the table after every move.
match       --games games, colours alternated: `gtp --playout-value N --playout-prior 1 --playout-rave K
            --playout-reply-pairs` against the same engine with --playout-replies, every pair of games from --opening-plies
            seeded random moves.  Wins and ms/move of both; a result within 40..60 is "no difference shown".
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
from reply_playout_bench import _event_ms, _policy_engine  # noqa: E402

PARTS = ("playouts", "update", "genmove", "match")


def _best(paths, reps):
    best, last = {}, {}
    for _ in range(reps):                                            # alternated
        for name, fn in paths.items():
            ms, last[name] = _event_ms(fn)
            best[name] = min(ms, best.get(name, ms))
    return best, last


def bench_playouts(games, reps, seed, pat, tac):
    dev = torch.device("cuda", 0)
    start = torch.from_numpy(reinforce.initial_positions(games)).to(dev)
    ctr = L.counters_to_device(rollout.default_counters(games, np.zeros(games, np.int32)), games, dev)
    w, t = pat.device(dev), tac.device(dev)
    tables = {"single": replies.ReplyTable.empty().device(dev).clone(), "pairs": replies.ReplyTable2.empty().device(dev).clone()}
    empty = {k: v.clone() for k, v in tables.items()}
    plays = {"single": (T.reply_playouts, T.reply_update), "pairs": (T.reply2_playouts, T.reply2_update)}
    for k, (play, update) in plays.items():                          # one batch, scored, folded into the table
        pos = start.clone()
        moves = play(pos, seed, ctr, w, t, tables[k], rollout.MAX_PLIES)[2]
        won = ((T.area_score(pos, L.KOMI) > 0) == L.black_to_move(start)).to(torch.uint8)
        update(start, moves, won, games, 1, tables[k])

    def run(play, table):
        return lambda: play(start.clone(), seed + 1, ctr, w, t, table, rollout.MAX_PLIES)[1]

    paths = {f"{k}_{kind}": run(plays[k][0], tabs[k]) for kind, tabs in (("empty", empty), ("learned", tables)) for k in plays}
    assert torch.equal(paths["single_empty"](), paths["pairs_empty"]())   # warm-up, and the same games
    paths["single_learned"](), paths["pairs_learned"]()
    best, plies = _best(paths, reps)
    return {"games": games, "pair_entries": int((tables["pairs"][:, :81] <= 80).sum()),
            "single_entries_of_pairs": int((tables["pairs"][:, 81] <= 80).sum()), "single_entries": int((tables["single"] <= 80).sum()),
            **{name: {"ms": best[name], "plies_mean": float(plies[name].float().mean())} for name in paths},
            "ratio_empty": best["pairs_empty"] / best["single_empty"], "ratio_learned": best["pairs_learned"] / best["single_learned"]}


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
        print(f"{games} games: all-255: single {r['single_empty']['ms']:.2f} ms, pairs x{r['ratio_empty']:.3f}; learned: single "
              f"{r['single_learned']['ms']:.2f} ms ({r['single_learned']['plies_mean']:.1f} plies), pairs x{r['ratio_learned']:.3f} "
              f"({r['pairs_learned']['plies_mean']:.1f} plies)", flush=True)
    return out


def bench_update(records, playouts, reps, seed):
    recs = torch.from_numpy(reinforce.initial_positions(records)).cuda()
    run = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", history=True)
    won, moves = run.won.to(torch.uint8).reshape(-1), run.moves
    single = replies.ReplyTable.empty().device(recs.device).clone()
    pairs = replies.ReplyTable2.empty().device(recs.device).clone()
    s1 = torch.empty((T.load().bkt_reply_scratch_bytes(records),), dtype=torch.uint8, device=recs.device)
    s2 = torch.empty((T.load().bkt_reply2_scratch_bytes(),), dtype=torch.uint8, device=recs.device)
    paths = {"reply_update": lambda: T.reply_update(recs, moves, won, records, playouts, single, s1),
             "reply2_update": lambda: T.reply2_update(recs, moves, won, records, playouts, pairs, s2)}
    for fn in paths.values():                                        # warm-up
        fn()
    best, _ = _best(paths, reps)
    assert torch.equal(pairs[:, 81], single)                          # plane 81 is the old update's table
    return {"records": records, "playouts": playouts, "max_plies": int(moves.shape[1]), "history_bytes": int(moves.numel() * 2),
            "reply_update_ms": best["reply_update"], "reply2_update_ms": best["reply2_update"],
            "scratch_bytes": {"reply_update": int(s1.numel()), "reply2_update": int(s2.numel())},
            "ratio": best["reply2_update"] / best["reply_update"]}


def part_update(args):
    out = {}
    for shape in args.shapes:
        records, playouts = (int(x) for x in shape.split("x"))
        out[shape] = r = bench_update(records, playouts, args.reps, args.seed)
        print(f"{shape}: bkt_reply_update {r['reply_update_ms']:.3f} ms, bkt_reply2_update {r['reply2_update_ms']:.3f} ms, "
              f"x{r['ratio']:.3f}", flush=True)
    return out


def _tree(args, **more):
    return NativeMCTS(Position(), None, None, playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                      playout_seed=args.seed, playout_rules=args.rules, **more)


def table_statistics(args):
    """One search with the option, not timed: per move, the plies its requests played, those the pair entries and the single
    entries decided, and the occupancy of both parts of the table after the move."""
    t = _tree(args, playout_reply_pairs=True)
    ev, seen = t.evaluator, {"plies": 0, "pair": 0, "single": 0}
    submit = ev.submit

    def counting(recs, n_policy):
        before = ev.replies.copy()
        h = submit(recs, n_policy)
        moves = rollout._numpy(h.run.moves)
        pair, single = replies.reply2_plies_of(before, np.ascontiguousarray(recs, np.uint8), moves, ev.playouts)
        seen["plies"] += int((np.cumsum(moves <= rollout.MOVE_NONE, 1) == 0).sum())
        seen["pair"], seen["single"] = seen["pair"] + pair, seen["single"] + single
        return h

    ev.submit = counting
    out = []
    for _ in range(args.genmoves):
        seen.update(plies=0, pair=0, single=0)
        t.rollout(args.rollouts)
        t.choose()
        out.append({"plies": seen["plies"], "pair_plies": seen["pair"], "single_plies": seen["single"],
                    "pair_occupancy": ev.replies.pairs_occupancy(), "single_occupancy": ev.replies.singles().occupancy()})
    t.close()
    return out


def part_genmove(args):
    kinds = {"pairs": {"playout_reply_pairs": True}, "singles": {"playout_replies": True}}
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
    plies, pair, single = (sum(m[k] for m in per_move) for k in ("plies", "pair_plies", "single_plies"))
    out = {"rollouts": args.rollouts, "playouts": args.playouts, "playout_rave": args.rave, "genmoves": args.genmoves,
           "pairs": best["pairs"], "singles": best["singles"], "ratio": best["pairs"]["ms_per_move"] / best["singles"]["ms_per_move"],
           "table": {"per_move": per_move, "plies": plies, "pair_plies": pair, "single_plies": single,
                     "pair_share": pair / max(plies, 1), "single_share": single / max(plies, 1)}}
    print(f"net-free genmove at {args.rollouts} rollouts: playout_reply_pairs {out['pairs']['ms_per_move']:.2f} ms/move, "
          f"playout_replies {out['singles']['ms_per_move']:.2f}, x{out['ratio']:.3f}; pairs decided "
          f"{100 * out['table']['pair_share']:.1f} % and singles {100 * out['table']['single_share']:.1f} % of {plies} plies; "
          f"occupancy (pairs, singles) {[(m['pair_occupancy'], m['single_occupancy']) for m in per_move]}", flush=True)
    return out


def part_match(args):
    from bokego_amd.gtp import NativeGTP

    def engine(name, **more):
        return match.InProcessEngine(NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=args.rollouts,
                                               playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                                               playout_rules=args.rules, **more), name=name)

    a, b = engine("pairs", playout_reply_pairs=True), engine("singles", playout_replies=True)
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["pairs_wins"]
    share = 100.0 * wins / args.games
    res.update(playout_rave=args.rave, rollouts=args.rollouts, playouts=args.playouts, opening_plies=args.opening_plies,
               seed=args.seed, verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("pairs win beyond the margin" if share > 60.0 else "pairs lose beyond the margin"))
    print(f"match: pairs {wins} : {res['singles_wins']} singles over {args.games} games -- {res['verdict']}; ms/move "
          f"{res['ms_per_move']['pairs']:.2f} / {res['ms_per_move']['singles']:.2f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--games", type=int, nargs="+", default=None, help="playouts: the batch sizes (4096 65536); match: the games (100)")
    ap.add_argument("--shapes", nargs="+", default=["1024x64", "81x64"], metavar="RxN", help="update: records x playouts")
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--genmoves", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--rave", type=float, default=4.0, metavar="K")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--rules", choices=("device", "host"), default="device")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_reply_bench.json"))
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

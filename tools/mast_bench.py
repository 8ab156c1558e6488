"""What the MAST playouts (bkt_move_value_playouts, bkt_move_value_update) cost and whether they win games, on
one MI355X.  tools/pair_reply_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps by HIP
events.  One threshold, the project's gate: the update against the same integers from torch, baseline / ours >= 1.0.

    python tools/mast_bench.py gate     [--shapes 1024x64] [--reps 3]
    python tools/mast_bench.py playouts [--games 4096 65536] [--reps 3]
    python tools/mast_bench.py search   [--shapes 1024x64 81x64] [--genmoves 8] [--rollouts 400] [--playouts 64] [--reps 3]
    python tools/mast_bench.py match    [--games 100] [--rollouts 400] [--playouts 64] [--opening-plies 4] [--seed 1] [--tau 0.25]
                                        [--pairs]
    (each with [--out profiles/mast_bench.json]: a part replaces its own entry of that file and leaves the others; search and
     match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

gate        bkt_move_value_update (two launches) over records x playouts histories from the empty board against the same
            update in torch on the history tensor: masks, two bincounts, the halvings as a fixed number of selects (no wait
            on the host), the index and the lut gather.  The results are compared for equality before anything is timed.
playouts    bkt_move_value_playouts against the kernel it wraps on the same rows, with fitted pattern and tactics tables:
            against bkt_tactical_playouts, and with a learned pair table against bkt_reply2_playouts; first with values all
            256 (what the staged table, the LDS read and the 64-bit multiply cost), then with a table learned from 20
            requests of 64 records x 64 playouts.  Time ratios, mean game lengths.  No threshold.
search      the update's time beside bkt_amaf_counts_sides' and bkt_reply2_update's on the same histories; ms per move of a
            net-free search (playout_prior=1, playout_rave=--rave) with and without playout_move_values, two trees
            alternated move by move; and after those moves the share of the table's entries with a play and its smallest
            and largest value.
match       --games games, colours alternated: the net-free RAVE engine with --playout-move-values TAU against the same
            engine without it (--pairs: both with --playout-reply-pairs), every pair of games from --opening-plies seeded
            random moves.  Wins and ms/move of both; a result within 40..60 is "no difference shown".
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
from bokego_amd import match, movevalues, reinforce, replies, rollout  # noqa: E402
from bokego_amd.mcts_native import NativeMCTS, Position  # noqa: E402
from pair_reply_bench import _best  # noqa: E402
from reply_playout_bench import _policy_engine  # noqa: E402

PARTS = ("gate", "playouts", "search", "match", "match_pairs", "match_tau")


def torch_update(recs, moves, won, playouts, counts, lut, k, limit, halvings):
    """bkt_move_value_update in torch, nothing waiting on the host -> (counts int64 [2,81,2], values int16 [2,81])."""
    m = moves.to(torch.int64)
    point = (torch.cumsum((m <= rollout.MOVE_NONE).to(torch.int32), 1) == 0) & (m >= 0) & (m <= 80)
    odd = torch.arange(m.shape[1], device=m.device) & 1
    c0 = (recs[:, L.OFF_TURN:L.OFF_TURN + 4].contiguous().view(torch.int32)[:, 0].to(torch.int64) & 1).repeat_interleave(playouts)
    flat = (c0[:, None] ^ odd[None, :]) * 81 + m.clamp(0, 80)
    mover_won = (won[:, None] != 0) == (odd[None, :] == 0)
    played = counts[..., 0].reshape(-1) + torch.bincount(flat[point], minlength=162)
    wins = counts[..., 1].reshape(-1) + torch.bincount(flat[point & mover_won], minlength=162)
    for _ in range(halvings if limit else 0):
        big = played >= limit
        played, wins = torch.where(big, played >> 1, played), torch.where(big, wins >> 1, wins)
    i = (64 * (2 * wins + k)) // (2 * (played + k))
    return torch.stack([played, wins], 1).view(2, 81, 2), lut[i.clamp(max=64)].view(2, 81)


def histories(records, playouts, seed):
    recs = torch.from_numpy(reinforce.initial_positions(records)).cuda()
    run = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", history=True)
    return recs, run.moves, run.won.to(torch.uint8).reshape(-1)


def part_gate(args):
    out = {}
    for shape in args.shapes:
        records, playouts = (int(x) for x in shape.split("x"))
        recs, moves, won = histories(records, playouts, args.seed)
        table = movevalues.MoveValueTable.empty()
        start, _, lut = (x.clone() for x in table.device(recs.device))
        k, limit = table.k, table.limit
        halvings = int(np.ceil(np.log2((limit + moves.numel()) / limit))) + 1
        counts, values = start.clone(), torch.zeros((2, 81), dtype=torch.int16, device=recs.device)
        scratch = torch.empty((T.load().bkt_move_value_scratch_bytes(records),), dtype=torch.uint8, device=recs.device)

        def ours():
            counts.copy_(start)
            return T.move_value_update(recs, moves, won, records, playouts, counts, values, lut, k, limit, scratch)

        def baseline():
            return torch_update(recs, moves, won, playouts, start, lut, k, limit, halvings)

        a, b = ours(), baseline()                                    # warm-up, and the same integers
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[0][..., 0].max()) < limit
        best, _ = _best({"ours": ours, "torch": baseline}, args.reps)
        out[shape] = r = {"records": records, "playouts": playouts, "max_plies": int(moves.shape[1]), "k": k, "limit": limit,
                          "plays": int(b[0][..., 0].sum()), "ours_ms": best["ours"], "torch_ms": best["torch"],
                          "speedup": best["torch"] / best["ours"], "gate_holds": best["torch"] / best["ours"] >= 1.0}
        print(f"gate {shape}: bkt_move_value_update {r['ours_ms']:.3f} ms, torch {r['torch_ms']:.3f} ms, x{r['speedup']:.2f} "
              f"({'holds' if r['gate_holds'] else 'FAILS'})", flush=True)
    return out


def learned_tables(pat, tac, seed, requests=20):
    """A move-value table and a pair reply table learned together from `requests` requests of 64 records x 64 playouts."""
    values, pairs = movevalues.MoveValueTable.empty(), replies.ReplyTable2.empty()
    recs = reinforce.initial_positions(64)
    for i in range(requests):
        rollout.playout_value(recs, 64, seed + i, patterns=pat, tactics=tac, replies=pairs, move_values=values)
    return values, pairs


def bench_playouts(games, reps, seed, pat, tac, learned, pairs):
    dev = torch.device("cuda", 0)
    start = torch.from_numpy(reinforce.initial_positions(games)).to(dev)
    ctr = L.counters_to_device(rollout.default_counters(games, np.zeros(games, np.int32)), games, dev)
    w, t = pat.device(dev), tac.device(dev)
    neutral = torch.full((2, 81), 256, dtype=torch.int16, device=dev)
    values, table2 = learned.device(dev)[1].clone(), pairs.device(dev).clone()
    cap = rollout.MAX_PLIES
    paths = {"tactical": lambda: T.tactical_playouts(start.clone(), seed, ctr, w, t, cap)[1],
             "values_neutral": lambda: T.move_value_playouts(start.clone(), seed, ctr, w, t, neutral, cap)[1],
             "values_learned": lambda: T.move_value_playouts(start.clone(), seed, ctr, w, t, values, cap)[1],
             "reply2": lambda: T.reply2_playouts(start.clone(), seed, ctr, w, t, table2, cap)[1],
             "reply2_values_neutral": lambda: T.move_value_playouts(start.clone(), seed, ctr, w, t, neutral, cap, replies2=table2)[1],
             "reply2_values_learned": lambda: T.move_value_playouts(start.clone(), seed, ctr, w, t, values, cap, replies2=table2)[1]}
    assert torch.equal(paths["tactical"](), paths["values_neutral"]())         # warm-up, and the same games
    assert torch.equal(paths["reply2"](), paths["reply2_values_neutral"]())
    paths["values_learned"](), paths["reply2_values_learned"]()
    best, plies = _best(paths, reps)
    return {"games": games, **{name: {"ms": best[name], "plies_mean": float(plies[name].float().mean())} for name in paths},
            "ratio_neutral": best["values_neutral"] / best["tactical"], "ratio_learned": best["values_learned"] / best["tactical"],
            "ratio_reply2_neutral": best["reply2_values_neutral"] / best["reply2"],
            "ratio_reply2_learned": best["reply2_values_learned"] / best["reply2"]}


def part_playouts(args):
    from tactical_playout_bench import fit_tables
    eng = _policy_engine()
    try:
        tables = fit_tables(eng, 4096, 101)
    finally:
        eng.close()
    learned, pairs = learned_tables(tables["patterns"], tables["tactics"], args.seed)
    out = {"learned": {"played_share": learned.occupancy() / 162, "min_value": int(learned.values.min()),
                       "max_value": int(learned.values.max()), "pair_entries": pairs.pairs_occupancy()}}
    for games in args.games:
        out[str(games)] = r = bench_playouts(games, args.reps, args.seed, tables["patterns"], tables["tactics"], learned, pairs)
        print(f"{games} games: tactical {r['tactical']['ms']:.2f} ms ({r['tactical']['plies_mean']:.1f} plies), values 256 "
              f"x{r['ratio_neutral']:.3f}, learned x{r['ratio_learned']:.3f} ({r['values_learned']['plies_mean']:.1f} plies); "
              f"reply2 {r['reply2']['ms']:.2f} ms, values 256 x{r['ratio_reply2_neutral']:.3f}, learned "
              f"x{r['ratio_reply2_learned']:.3f} ({r['reply2_values_learned']['plies_mean']:.1f} plies)", flush=True)
    return out


def _tree(args, **more):
    return NativeMCTS(Position(), None, None, playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                      playout_seed=args.seed, playout_rules=args.rules, **more)


def part_search(args):
    out = {"update": {}}
    for shape in args.shapes if args.rules == "device" else ():
        records, playouts = (int(x) for x in shape.split("x"))
        recs, moves, won = histories(records, playouts, args.seed)
        counts, values, lut = (x.clone() for x in movevalues.MoveValueTable.empty().device(recs.device))
        pairs = replies.ReplyTable2.empty().device(recs.device).clone()
        s1 = torch.empty((T.load().bkt_move_value_scratch_bytes(records),), dtype=torch.uint8, device=recs.device)
        s2 = torch.empty((T.load().bkt_reply2_scratch_bytes(),), dtype=torch.uint8, device=recs.device)
        paths = {"move_value_update": lambda: T.move_value_update(recs, moves, won, records, playouts, counts, values, lut, 16, 16384, s1),
                 "amaf_counts_sides": lambda: T.amaf_counts_sides(moves, won, records, playouts),
                 "reply2_update": lambda: T.reply2_update(recs, moves, won, records, playouts, pairs, s2)}
        for fn in paths.values():
            fn()
        best, _ = _best(paths, args.reps)
        out["update"][shape] = {"max_plies": int(moves.shape[1]), **{f"{name}_ms": ms for name, ms in best.items()}}
        print(f"{shape}: " + ", ".join(f"{name} {ms:.3f} ms" for name, ms in best.items()), flush=True)
    kinds = {"move_values": {"playout_move_values": args.tau}, "plain": {}}
    best, table = {}, None
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
        mv = trees["move_values"].evaluator.move_values
        table = {"played_share": mv.occupancy() / 162, "min_value": int(mv.values.min()), "max_value": int(mv.values.max()),
                 "max_played": int(mv.counts[..., 0].max())}
        for k, t in trees.items():
            t.close()
            mean = float(np.mean(ms[k]))
            if k not in best or mean < best[k]["ms_per_move"]:
                best[k] = {"ms_per_move": mean, "ms_each": ms[k]}
    out.update(rollouts=args.rollouts, playouts=args.playouts, playout_rave=args.rave, genmoves=args.genmoves, tau=args.tau,
               move_values=best["move_values"], plain=best["plain"], table_after=table,
               ratio=best["move_values"]["ms_per_move"] / best["plain"]["ms_per_move"])
    print(f"net-free genmove at {args.rollouts} rollouts: playout_move_values {best['move_values']['ms_per_move']:.2f} ms/move, "
          f"without {best['plain']['ms_per_move']:.2f}, x{out['ratio']:.3f}; the table after {args.genmoves} moves: {table}", flush=True)
    return out


def part_match(args):
    from bokego_amd.gtp import NativeGTP

    def engine(name, **more):
        if args.pairs:
            more["playout_reply_pairs"] = True
        return match.InProcessEngine(NativeGTP(Position(), None, None, no_sim=True, time_lim=None, n_rollouts=args.rollouts,
                                               playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                                               playout_rules=args.rules, **more), name=name)

    a, b = engine("mast", playout_move_values=args.tau), engine("plain")
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["mast_wins"]
    share = 100.0 * wins / args.games
    res.update(playout_rave=args.rave, rollouts=args.rollouts, playouts=args.playouts, opening_plies=args.opening_plies,
               seed=args.seed, tau=args.tau, reply_pairs_on_both_sides=bool(args.pairs),
               verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("move values win beyond the margin" if share > 60.0 else "move values lose beyond the margin"))
    print(f"match (tau {args.tau}{', reply pairs on both sides' if args.pairs else ''}): mast {wins} : {res['plain_wins']} plain over "
          f"{args.games} games -- {res['verdict']}; ms/move {res['ms_per_move']['mast']:.2f} / {res['ms_per_move']['plain']:.2f}",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS[:4])
    ap.add_argument("--games", type=int, nargs="+", default=None, help="playouts: the batch sizes (4096 65536); match: the games (100)")
    ap.add_argument("--shapes", nargs="+", default=None, metavar="RxN", help="gate (1024x64), search (1024x64 81x64): records x playouts")
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--genmoves", type=int, default=8)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--rave", type=float, default=4.0, metavar="K")
    ap.add_argument("--tau", type=float, default=movevalues.DEFAULT_TAU)
    ap.add_argument("--pairs", action="store_true", help="match: --playout-reply-pairs on both sides")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--rules", choices=("device", "host"), default="device")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mast_bench.json"))
    args = ap.parse_args()
    if args.part == "match":
        args.games = 100 if args.games is None else args.games[0]
    elif args.games is None:
        args.games = [4096, 65536]
    if args.shapes is None:
        args.shapes = ["1024x64"] if args.part == "gate" else ["1024x64", "81x64"]
    out = {part: "not measured" for part in PARTS}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0) if args.rules == "device" else "none (host rules: a dry run)"
    key = args.part if args.part != "match" else ("match_pairs" if args.pairs else "match_tau" if args.tau != movevalues.DEFAULT_TAU
                                                  else "match")
    out[key] = {"gate": part_gate, "playouts": part_playouts, "search": part_search, "match": part_match}[args.part](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""What the NAST playouts (bkt_move_context_playouts, bkt_move_context_update) cost and whether they win games, on
one MI355X.  tools/game_move_values_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps by HIP
events; every part a process of its own.  One threshold, the project's gate: the update against the same integers from
torch, baseline / ours >= 1.0.

    python tools/nast_bench.py gate     [--shapes 1024x64] [--reps 3]
    python tools/nast_bench.py playouts [--games 4096 65536] [--reps 3]
    python tools/nast_bench.py update   [--shapes 1024x64 81x64] [--reps 3]
    python tools/nast_bench.py search   [--genmoves 8] [--rollouts 400] [--playouts 64] [--reps 3]
    python tools/nast_bench.py match    [--games 100] [--rollouts 400] [--playouts 64] [--opening-plies 4] [--seed 1] [--pairs]
    python tools/nast_bench.py all      [--limit SECONDS] [--skip-matches]
    (each with [--out profiles/nast_bench.json]: a part replaces its own entry of that file and leaves the others; search and
     match take --rules host, the playouts on the host mirror: a dry run where there is no GPU, not a measurement)

gate        bkt_move_context_update (three launches) over records x playouts histories, 400 plies wide, against the same
            update in torch on the history tensor: masks, bincounts over the 13,284 entries, the halvings as a fixed number of
            selects (no wait on the host), the two indices and the lut gather.  Equality is checked before anything is timed.
playouts    bkt_move_context_playouts against bkt_move_value_playouts on the same rows with fitted pattern and tactics
            tables, alone and under a learned pair table: with values all 256, and with a move-context table learned from 20
            requests of 64 records x 64 playouts against its own plane 81.  The baseline is timed twice under two names: the
            ratio of those two is the spread the other ratios are read beside.  No threshold: this is the number that says
            whether the per-ply read from L2 is visible.
update      the update's time beside bkt_move_value_update's and bkt_reply2_update's on the same histories.
search      ms per move of a net-free search (playout_prior=1, playout_rave=--rave) with and without playout_move_contexts, two
            trees alternated move by move; after those moves the share of context entries at or above min_plays and the range
            of the learned values.
match       --games games, colours alternated: the net-free RAVE engine with --playout-move-contexts against the same engine
            with --playout-move-values (--pairs: both with --playout-reply-pairs), every pair of games from --opening-plies
            seeded random moves.  Wins and ms/move of both; a result within 40..60 is "no difference shown".
all         the parts above as child processes, one after the other, each under --limit seconds; the first one that fails
            or runs out of time ends the run.
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
from bokego_amd import match, movecontexts, movevalues, reinforce, replies, rollout  # noqa: E402
from bokego_amd.mcts_native import NativeMCTS, Position  # noqa: E402

PARTS = ("gate", "playouts", "update", "search", "match", "match_pairs")
ENTRIES = 2 * 82 * 81


def _best(paths, reps):
    from pair_reply_bench import _best as best
    return best(paths, reps)[0]


def torch_update(recs, moves, won, playouts, counts, lut, k, limit, min_plays, halvings):
    """bkt_move_context_update in torch, nothing waiting on the host -> (counts int64 [2,82,81,2], values int16 [2,82,81])."""
    m = moves.to(torch.int64)
    point = (torch.cumsum((m <= rollout.MOVE_NONE).to(torch.int32), 1) == 0) & (m >= 0) & (m <= 80)
    odd = torch.arange(m.shape[1], device=m.device) & 1
    c0 = (recs[:, L.OFF_TURN:L.OFF_TURN + 4].contiguous().view(torch.int32)[:, 0].to(torch.int64) & 1).repeat_interleave(playouts)
    last = recs[:, L.OFF_LAST_MOVE:L.OFF_LAST_MOVE + 2].contiguous().view(torch.int16)[:, 0].to(torch.int64).repeat_interleave(playouts)
    prev = torch.cat([last[:, None], m[:, :-1]], 1)
    context = (prev >= 0) & (prev <= 80)
    base = (c0[:, None] ^ odd[None, :]) * (82 * 81) + m.clamp(0, 80)
    plain, keyed = base + 81 * 81, base + 81 * prev.clamp(0, 80)
    mover_won = (won[:, None] != 0) == (odd[None, :] == 0)
    keyed_point = point & context
    played = counts[..., 0].reshape(-1) + torch.bincount(plain[point], minlength=ENTRIES) + torch.bincount(keyed[keyed_point], minlength=ENTRIES)
    wins = counts[..., 1].reshape(-1) + torch.bincount(plain[point & mover_won], minlength=ENTRIES) \
        + torch.bincount(keyed[keyed_point & mover_won], minlength=ENTRIES)
    for _ in range(halvings if limit else 0):
        big = played >= limit
        played, wins = torch.where(big, played >> 1, played), torch.where(big, wins >> 1, wins)
    i = ((64 * (2 * wins + k)) // (2 * (played + k))).clamp(max=64).view(2, 82, 81)
    i1 = i[:, 81:82]
    index = torch.where(played.view(2, 82, 81) >= min_plays, (i1 + i) >> 1, i1.expand(2, 82, 81)).clone()
    index[:, 81] = i[:, 81]
    return torch.stack([played, wins], 1).view(2, 82, 81, 2), lut[index]


def histories(records, playouts, seed):
    recs = torch.from_numpy(reinforce.initial_positions(records)).cuda()
    run = rollout._playouts(recs, playouts, L.seed_u64(seed), rules="device", history=True)
    return recs, run.moves, run.won.to(torch.uint8).reshape(-1)


def part_gate(args):
    out = {}
    for shape in args.shapes:
        records, playouts = (int(x) for x in shape.split("x"))
        recs, moves, won = histories(records, playouts, args.seed)
        table = movecontexts.MoveContextTable.empty()
        start, _, lut = (x.clone() for x in table.device(recs.device))
        k, limit, min_plays = table.k, table.limit, table.min_plays
        halvings = int(np.ceil(np.log2((limit + moves.numel()) / limit))) + 1
        counts, values = start.clone(), torch.zeros((2, 82, 81), dtype=torch.int16, device=recs.device)
        scratch = torch.empty((T.move_context_scratch_bytes(records),), dtype=torch.uint8, device=recs.device)

        def ours():
            counts.copy_(start)
            return T.move_context_update(recs, moves, won, records, playouts, counts, values, lut, k, limit, min_plays, scratch)

        def baseline():
            return torch_update(recs, moves, won, playouts, start, lut, k, limit, min_plays, halvings)

        a, b = ours(), baseline()                                    # warm-up, and the same integers
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[0][..., 0].max()) < limit
        best = _best({"ours": ours, "torch": baseline}, args.reps)
        out[shape] = r = {"records": records, "playouts": playouts, "max_plies": int(moves.shape[1]), "k": k, "limit": limit,
                          "min_plays": min_plays, "plays": int(b[0][:, 81, :, 0].sum()), "context_plays": int(b[0][:, :81, :, 0].sum()),
                          "ours_ms": best["ours"], "torch_ms": best["torch"], "speedup": best["torch"] / best["ours"],
                          "gate_holds": best["torch"] / best["ours"] >= 1.0}
        print(f"gate {shape}: bkt_move_context_update {r['ours_ms']:.3f} ms, torch {r['torch_ms']:.3f} ms, x{r['speedup']:.2f} "
              f"({'holds' if r['gate_holds'] else 'FAILS'})", flush=True)
    return out


def learned_tables(pat, tac, seed, requests=20):
    """A move-context table and a pair reply table learned together from `requests` requests of 64 records x 64 playouts."""
    contexts, pairs = movecontexts.MoveContextTable.empty(), replies.ReplyTable2.empty()
    recs = reinforce.initial_positions(64)
    for i in range(requests):
        rollout.playout_value(recs, 64, seed + i, patterns=pat, tactics=tac, replies=pairs, move_values=contexts)
    return contexts, pairs


def bench_playouts(games, reps, seed, pat, tac, learned, pairs):
    dev = torch.device("cuda", 0)
    start = torch.from_numpy(reinforce.initial_positions(games)).to(dev)
    ctr = L.counters_to_device(rollout.default_counters(games, np.zeros(games, np.int32)), games, dev)
    w, t = pat.device(dev), tac.device(dev)
    neutral, neutral_c = (torch.full(s, 256, dtype=torch.int16, device=dev) for s in ((2, 81), (2, 82, 81)))
    contexts, table2 = learned.device(dev)[1].clone(), pairs.device(dev).clone()
    plane = contexts[:, 81].contiguous()                              # the baseline's learned table: plane 81 of ours
    cap = rollout.MAX_PLIES
    mv, mc = T.move_value_playouts, T.move_context_playouts
    paths = {"values_neutral": lambda: mv(start.clone(), seed, ctr, w, t, neutral, cap)[1],
             "contexts_neutral": lambda: mc(start.clone(), seed, ctr, w, t, neutral_c, cap)[1],
             "values_neutral_again": lambda: mv(start.clone(), seed, ctr, w, t, neutral, cap)[1],
             "values_learned": lambda: mv(start.clone(), seed, ctr, w, t, plane, cap)[1],
             "contexts_learned": lambda: mc(start.clone(), seed, ctr, w, t, contexts, cap)[1],
             "pairs_values_neutral": lambda: mv(start.clone(), seed, ctr, w, t, neutral, cap, replies2=table2)[1],
             "pairs_contexts_neutral": lambda: mc(start.clone(), seed, ctr, w, t, neutral_c, cap, replies2=table2)[1],
             "pairs_values_neutral_again": lambda: mv(start.clone(), seed, ctr, w, t, neutral, cap, replies2=table2)[1],
             "pairs_values_learned": lambda: mv(start.clone(), seed, ctr, w, t, plane, cap, replies2=table2)[1],
             "pairs_contexts_learned": lambda: mc(start.clone(), seed, ctr, w, t, contexts, cap, replies2=table2)[1]}
    assert torch.equal(paths["values_neutral"](), paths["contexts_neutral"]())           # warm-up, and the same games
    assert torch.equal(paths["pairs_values_neutral"](), paths["pairs_contexts_neutral"]())
    best = _best(paths, reps)
    return {"games": games, **{f"{name}_ms": ms for name, ms in best.items()},
            "ratio_neutral": best["contexts_neutral"] / best["values_neutral"],
            "ratio_learned": best["contexts_learned"] / best["values_learned"],
            "baseline_spread": best["values_neutral_again"] / best["values_neutral"],
            "ratio_pairs_neutral": best["pairs_contexts_neutral"] / best["pairs_values_neutral"],
            "ratio_pairs_learned": best["pairs_contexts_learned"] / best["pairs_values_learned"],
            "baseline_spread_pairs": best["pairs_values_neutral_again"] / best["pairs_values_neutral"]}


def part_playouts(args):
    from reply_playout_bench import _policy_engine
    from tactical_playout_bench import fit_tables
    eng = _policy_engine()
    try:
        tables = fit_tables(eng, 4096, 101)
    finally:
        eng.close()
    learned, pairs = learned_tables(tables["patterns"], tables["tactics"], args.seed)
    out = {"learned": {"played_share": int((learned.counts[:, 81, :, 0] > 0).sum()) / 162,
                       "context_qualified_share": learned.qualified() / (2 * 81 * 81), "min_value": int(learned.values.min()),
                       "max_value": int(learned.values.max()), "pair_entries": pairs.pairs_occupancy()}}
    for games in args.games:
        out[str(games)] = r = bench_playouts(games, args.reps, args.seed, tables["patterns"], tables["tactics"], learned, pairs)
        print(f"{games} games: bkt_move_value_playouts {r['values_neutral_ms']:.2f} ms, contexts all 256 x{r['ratio_neutral']:.3f}, "
              f"learned x{r['ratio_learned']:.3f} (the baseline against itself x{r['baseline_spread']:.3f}); under pairs "
              f"{r['pairs_values_neutral_ms']:.2f} ms, all 256 x{r['ratio_pairs_neutral']:.3f}, learned x{r['ratio_pairs_learned']:.3f} "
              f"(x{r['baseline_spread_pairs']:.3f})", flush=True)
    return out


def part_update(args):
    out = {}
    for shape in args.shapes:
        records, playouts = (int(x) for x in shape.split("x"))
        recs, moves, won = histories(records, playouts, args.seed)
        cc, cv, lut = (x.clone() for x in movecontexts.MoveContextTable.empty().device(recs.device))
        vc, vv, _ = (x.clone() for x in movevalues.MoveValueTable.empty().device(recs.device))
        pairs = replies.ReplyTable2.empty().device(recs.device).clone()
        s0 = torch.empty((T.move_context_scratch_bytes(records),), dtype=torch.uint8, device=recs.device)
        s1 = torch.empty((T.load().bkt_move_value_scratch_bytes(records),), dtype=torch.uint8, device=recs.device)
        s2 = torch.empty((T.load().bkt_reply2_scratch_bytes(),), dtype=torch.uint8, device=recs.device)
        paths = {"move_context_update": lambda: T.move_context_update(recs, moves, won, records, playouts, cc, cv, lut, 16, 16384, 8, s0),
                 "move_value_update": lambda: T.move_value_update(recs, moves, won, records, playouts, vc, vv, lut, 16, 16384, s1),
                 "reply2_update": lambda: T.reply2_update(recs, moves, won, records, playouts, pairs, s2)}
        best = _best(paths, args.reps)
        out[shape] = {"max_plies": int(moves.shape[1]), **{f"{name}_ms": ms for name, ms in best.items()}}
        print(f"{shape}: " + ", ".join(f"{name} {ms:.3f} ms" for name, ms in best.items()), flush=True)
    return out


def _tree(args, **more):
    return NativeMCTS(Position(), None, None, playout_value=args.playouts, playout_prior=1.0, playout_rave=args.rave,
                      playout_seed=args.seed, playout_rules=args.rules, **more)


def part_search(args):
    kinds = {"move_contexts": {"playout_move_contexts": args.tau}, "plain": {}}
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
        mc = trees["move_contexts"].evaluator.move_values
        table = {"played_share": int((mc.counts[:, 81, :, 0] > 0).sum()) / 162, "min_plays": mc.min_plays,
                 "context_played_share": int((mc.counts[:, :81, :, 0] > 0).sum()) / (2 * 81 * 81),
                 "context_qualified_share": mc.qualified() / (2 * 81 * 81), "min_value": int(mc.values.min()),
                 "max_value": int(mc.values.max()), "max_played": int(mc.counts[..., 0].max())}
        for k, t in trees.items():
            t.close()
            mean = float(np.mean(ms[k]))
            if k not in best or mean < best[k]["ms_per_move"]:
                best[k] = {"ms_per_move": mean, "ms_each": ms[k]}
    out = dict(rollouts=args.rollouts, playouts=args.playouts, playout_rave=args.rave, genmoves=args.genmoves, tau=args.tau,
               move_contexts=best["move_contexts"], plain=best["plain"], table_after=table,
               ratio=best["move_contexts"]["ms_per_move"] / best["plain"]["ms_per_move"])
    print(f"net-free genmove at {args.rollouts} rollouts: playout_move_contexts {best['move_contexts']['ms_per_move']:.2f} ms/move, "
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

    a, b = engine("nast", playout_move_contexts=args.tau), engine("mast", playout_move_values=args.tau)
    res = match.play_match(a, b, args.games, L.KOMI, None, args.opening_plies, args.seed, progress=sys.stderr)
    res.pop("records")
    wins = res["nast_wins"]
    share = 100.0 * wins / args.games
    res.update(playout_rave=args.rave, rollouts=args.rollouts, playouts=args.playouts, opening_plies=args.opening_plies,
               seed=args.seed, tau=args.tau, reply_pairs_on_both_sides=bool(args.pairs),
               verdict="no difference shown" if 40.0 <= share <= 60.0 else
               ("move contexts win beyond the margin" if share > 60.0 else "move contexts lose beyond the margin"))
    print(f"match ({'reply pairs on both sides' if args.pairs else 'no reply table'}): nast {wins} : {res['mast_wins']} mast over "
          f"{args.games} games -- {res['verdict']}; ms/move {res['ms_per_move']['nast']:.2f} / {res['ms_per_move']['mast']:.2f}",
          flush=True)
    return res


def run_all(args):
    """Every part as a child process under --limit seconds; the first failure ends the run (nothing more starts on the GPU)."""
    parts = [["gate"], ["playouts"], ["update"], ["search"]] + ([] if args.skip_matches else [["match"], ["match", "--pairs"]])
    for part in parts:
        cmd = [sys.executable, os.path.abspath(__file__), *part, "--out", args.out, "--rules", args.rules]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"{' '.join(part)} ended with {rc}: the parts after it are not run", flush=True)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS[:5] + ("all",))
    ap.add_argument("--games", type=int, nargs="+", default=None, help="playouts: the batch sizes (4096 65536); match: the games (100)")
    ap.add_argument("--shapes", nargs="+", default=None, metavar="RxN", help="gate (1024x64), update (1024x64 81x64): records x playouts")
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
    ap.add_argument("--limit", type=float, default=900.0, help="all: the time limit of each part, seconds")
    ap.add_argument("--skip-matches", action="store_true", help="all: without the two matches (they read 'not measured')")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nast_bench.json"))
    args = ap.parse_args()
    if args.part == "all":
        sys.exit(run_all(args))
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
    key = "match_pairs" if args.part == "match" and args.pairs else args.part
    out[key] = {"gate": part_gate, "playouts": part_playouts, "update": part_update, "search": part_search,
                "match": part_match}[args.part](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

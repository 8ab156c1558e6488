"""What a move-value table per game costs (bkt_move_value_playouts_tables, bkt_move_value_update_tables), on one
MI355X.  By tools/game_pair_tables_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps, by HIP
events; every part is a process of its own.  Only the gate has a threshold; everything else is recorded.

    python tools/game_move_values_bench.py gate      [--games 8 64 512] [--reps 3]
    python tools/game_move_values_bench.py playouts  [--rows 4096 65536] [--reps 3]
    python tools/game_move_values_bench.py update    [--records 1536] [--playouts 64] [--reps 3]
    python tools/game_move_values_bench.py selfplay  [--games 64] [--rollouts 400] [--playouts 64]
    (each with [--out profiles/game_move_values_bench.json]: a part replaces its own entry of that file and leaves the others)

gate        G games x 3 records x 64 playouts, tables learned from a first batch.  New: one bkt_move_value_playouts_tables
            (one per 65,536 rows: two at 512 games) plus one bkt_move_value_update_tables.  Baseline, what the library offered
            before: G bkt_move_value_playouts plus G bkt_move_value_update, one pair per game, on one stream.  Both leave the
            same tables (checked first).  ratio = baseline / new must be >= 1.0 at 64 games; 8 and 512 are reported.
playouts    bkt_move_value_playouts_tables with 64 copies of one learned table (slot = row % 64) against
            bkt_move_value_playouts with that table on the same rows, at every size of --rows, alone, under single reply
            tables per game and under pair reply tables per game; the same games (checked).  The baseline is timed twice under
            two names: the ratio of those two is the run-to-run spread the ratios are read beside.
update      bkt_move_value_update_tables with 1, 64 and 512 tables (slot = record % tables) against bkt_move_value_update, on
            --records x --playouts real histories.
selfplay    --games games x --rollouts rollouts, playout_value --playouts, playout_prior 1, on the Python loop: plain; a
            move-value table per game; rave=4 with a pair reply table and a move-value table per game.  Seconds, games/min,
            mean game length, black/white wins, and the range of the learned values at the end.
No strength figure of the pool engine is measured here: the pools have no match harness.  A part that did not run reads "not
measured".
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]

from bokego_amd import _trainlib as T  # noqa: E402
from bokego_amd import movevalues, replies, rollout, selfplay  # noqa: E402
from bokego_amd import lockstep as L  # noqa: E402
from game_pair_tables_bench import _best, _chunks, _won, golden_records  # noqa: E402

PARTS = ("gate", "playouts", "update", "selfplay")
DEV = torch.device("cuda", 0)
CAP = rollout.MAX_PLIES
K, LIMIT = movevalues.DEFAULT_K, movevalues.DEFAULT_LIMIT


def _lut():
    return torch.from_numpy(movevalues.lut_of(movevalues.DEFAULT_TAU).view(np.int16).copy()).to(DEV)


def _empty(count=None):
    shape = () if count is None else (count,)
    return (torch.zeros(shape + (2, 81, 2), dtype=torch.int64, device=DEV),
            torch.full(shape + (2, 81), movevalues.NEUTRAL, dtype=torch.int16, device=DEV))


def bench_gate(games, n, reps, seed):
    R = 3 * games
    recs = torch.from_numpy(golden_records(R)).to(DEV)
    start = recs.repeat_interleave(n, 0)
    ctr = L.value_counters_device(recs, n)
    slots = (torch.arange(R, device=DEV, dtype=torch.int32) // 3).contiguous()
    row_slots = slots.repeat_interleave(n).contiguous()
    lut = _lut()
    l_counts, l_values = _empty(games)

    def play_all(values, pos, key):
        return torch.cat([T.move_value_playouts(pos[s:s + T.MAX_BATCH], key, ctr[s:s + T.MAX_BATCH], None, None, values, CAP,
                                                slots=row_slots[s:s + T.MAX_BATCH])[2] for s in _chunks(len(pos))])

    pos = start.clone()                                               # the first batch: scored, folded into the tables
    moves = play_all(l_values, pos, seed)
    T.move_value_update(recs, moves, _won(pos, recs, n), R, n, l_counts, l_values, lut, K, LIMIT, slots=slots)
    pos = start.clone()                                               # who wins the timed batch (its playouts are fixed by the tables)
    play_all(l_values, pos, seed + 1)
    won = _won(pos, recs, n)
    many = torch.empty((T.load().bkt_move_value_tables_scratch_bytes(R, games),), dtype=torch.uint8, device=DEV)
    single = torch.empty((T.load().bkt_move_value_scratch_bytes(3),), dtype=torch.uint8, device=DEV)
    counts, values, work = l_counts.clone(), l_values.clone(), start.clone()

    def reset():
        counts.copy_(l_counts)
        values.copy_(l_values)
        work.copy_(start)

    def new():
        T.move_value_update(recs, play_all(values, work, seed + 1), won, R, n, counts, values, lut, K, LIMIT, many, slots=slots)

    def baseline():
        for g in range(games):
            r, w = slice(3 * g, 3 * g + 3), slice(3 * n * g, 3 * n * (g + 1))
            m = T.move_value_playouts(work[w], seed + 1, ctr[w], None, None, values[g], CAP)[2]
            T.move_value_update(recs[r], m, won[w], 3, n, counts[g], values[g], lut, K, LIMIT, single)

    after = {}
    for name, fn in (("new", new), ("baseline", baseline)):            # the same tables either way
        reset()
        fn()
        after[name] = (counts.clone(), values.clone())
    assert all(torch.equal(a, b) for a, b in zip(after["new"], after["baseline"])) and not torch.equal(after["new"][0], l_counts)
    best = _best({"new": new, "baseline": baseline}, reps, reset)
    v = l_values.cpu().numpy().view(np.uint16)
    return {"games": games, "records": R, "playouts": n, "rows": R * n, "playout_launches_new": len(_chunks(R * n)),
            "values_min": int(v.min()), "values_max": int(v.max()), "new_ms": best["new"], "baseline_ms": best["baseline"],
            "ratio": best["baseline"] / best["new"]}


def part_gate(args):
    out = {}
    for games in args.games:
        out[str(games)] = r = bench_gate(games, args.playouts, args.reps, args.seed)
        print(f"{games} games x 3 x {args.playouts}: one launch pair {r['new_ms']:.3f} ms, {games} pairs {r['baseline_ms']:.3f} ms, "
              f"x{r['ratio']:.2f}", flush=True)
    if "64" in out:
        out["gate"] = {"ratio_at_64": out["64"]["ratio"], "holds": bool(out["64"]["ratio"] >= 1.0)}
        print(f"gate (ratio >= 1.0 at 64 games): {'holds' if out['gate']['holds'] else 'FAILS'}", flush=True)
    return out


def _learned(recs, n, seed):
    """One move-value table and one pair reply table learned from n uniform playouts of recs."""
    counts, values = _empty()
    pairs = torch.full((2, 82, 81), replies.NONE, dtype=torch.uint8, device=DEV)
    pos = recs.repeat_interleave(n, 0)
    moves = T.random_playouts(pos, seed, L.value_counters_device(recs, n), CAP)[2]
    won = _won(pos, recs, n)
    T.move_value_update(recs, moves, won, len(recs), n, counts, values, _lut(), K, LIMIT)
    T.reply2_update(recs, moves, won, len(recs), n, pairs)
    return values, pairs


def part_playouts(args):
    out = {}
    for rows in args.rows:
        start = torch.from_numpy(golden_records(rows)).to(DEV)
        ctr = L.counters_to_device(rollout.default_counters(rows, rollout.record_turns(start.cpu().numpy())), rows, DEV)
        values, pairs = _learned(start[:64].contiguous(), 16, args.seed)
        singles = pairs[:, 81].contiguous()
        spread = (torch.arange(rows, device=DEV, dtype=torch.int32) % 64).contiguous()
        v64 = values[None].repeat(64, 1, 1).contiguous()
        forms = {"alone": ({}, {}), "singles": (dict(replies=singles), dict(replies=singles[None].repeat(64, 1, 1).contiguous())),
                 "pairs": (dict(replies2=pairs), dict(replies2=pairs[None].repeat(64, 1, 1, 1).contiguous()))}
        out[str(rows)] = res = {"rows": rows, "values_min": int(values.cpu().numpy().view(np.uint16).min()),
                                "values_max": int(values.cpu().numpy().view(np.uint16).max())}
        for form, (one, many) in forms.items():
            paths = {"single": lambda one=one: T.move_value_playouts(start.clone(), args.seed, ctr, None, None, values, CAP, **one),
                     "tables_64": lambda many=many: T.move_value_playouts(start.clone(), args.seed, ctr, None, None, v64, CAP,
                                                                          slots=spread, **many),
                     "single_again": lambda one=one: T.move_value_playouts(start.clone(), args.seed, ctr, None, None, values, CAP, **one)}
            assert all(torch.equal(a, b) for a, b in zip(paths["tables_64"](), paths["single"]()))   # the same games
            best = _best(paths, args.reps)
            res[form] = r = {**{f"{k}_ms": v for k, v in best.items()}, "ratio_tables_64": best["tables_64"] / best["single"],
                             "baseline_spread": best["single_again"] / best["single"]}
            print(f"{rows} rows, {form}: bkt_move_value_playouts {best['single']:.3f} ms, 64 tables x{r['ratio_tables_64']:.3f} "
                  f"(the baseline against itself x{r['baseline_spread']:.3f})", flush=True)
    return out


def part_update(args):
    R, n = args.records, args.playouts
    recs = torch.from_numpy(golden_records(R)).to(DEV)
    pos = recs.repeat_interleave(n, 0)
    moves = torch.cat([T.random_playouts(pos[s:s + T.MAX_BATCH], args.seed, L.value_counters_device(recs, n)[s:s + T.MAX_BATCH],
                                         CAP)[2] for s in _chunks(R * n)])
    won = _won(pos, recs, n)
    lut = _lut()
    scratch = torch.empty((T.load().bkt_move_value_scratch_bytes(R),), dtype=torch.uint8, device=DEV)
    c1, v1 = _empty()
    paths = {"single": lambda: T.move_value_update(recs, moves, won, R, n, c1, v1, lut, K, LIMIT, scratch)}
    for count in (1, 64, 512):
        c, v = _empty(count)
        slots = (torch.arange(R, device=DEV, dtype=torch.int32) % count).contiguous()
        paths[f"tables_{count}"] = (lambda c=c, v=v, s=slots: T.move_value_update(recs, moves, won, R, n, c, v, lut, K, LIMIT, scratch, slots=s))
    best = _best(paths, args.reps)
    out = {"records": R, "playouts": n, "max_plies": CAP, **{f"{name}_ms": ms for name, ms in best.items()}}
    print(f"{R} x {n} histories: bkt_move_value_update {best['single']:.4f} ms; bkt_move_value_update_tables 1 / 64 / 512: "
          f"{best['tables_1']:.4f} / {best['tables_64']:.4f} / {best['tables_512']:.4f} ms", flush=True)
    return out


def part_selfplay(args):
    base = dict(prior=1.0, seed=args.seed)
    kw = dict(n_games=args.games, rollouts=args.rollouts)
    kinds = {"plain_python_loop": (dict(), dict(native_loop=False)),
             "game_move_values": (dict(move_value_games=args.games), dict()),
             "game_rave_reply_pairs_move_values": (dict(rave=True, pair_games=args.games, move_value_games=args.games), dict(rave=4.0))}
    selfplay.self_play(rollout.PlayoutEvaluator(None, args.playouts, **base), n_games=2, rollouts=8, max_turns=4)     # warm-up
    out = {"games": args.games, "rollouts": args.rollouts, "playouts": args.playouts}
    for name, (ev_kw, sp_kw) in kinds.items():
        ev = rollout.PlayoutEvaluator(None, args.playouts, **base, **ev_kw)
        torch.cuda.synchronize()
        local, total = selfplay.self_play(ev, **kw, **sp_kw)
        out[name] = r = {"seconds": local["seconds"], "games_per_min": args.games / local["seconds"] * 60,
                         "mean_game_length": total["plies"] / max(total["games"], 1), "black_wins": total["black_wins"],
                         "white_wins": total["white_wins"], "steps": local["steps"], "native_loop": local["native_loop"]}
        if ev.move_values is not None:
            v = ev.move_values.values
            r["values_min"], r["values_max"] = int(v.min()), int(v.max())
            r["entries_played_mean"] = float(np.mean(ev.move_values.occupancy()))
        print(f"{name}: {r['seconds']:.1f} s, {r['games_per_min']:.1f} games/min, {r['mean_game_length']:.1f} plies/game, "
              f"B {r['black_wins']:.0f} : W {r['white_wins']:.0f}" +
              (f", values {r['values_min']}..{r['values_max']}" if "values_min" in r else ""), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--games", type=int, nargs="+", default=None, help="gate: the pool sizes (8 64 512); selfplay: the games (64)")
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--records", type=int, default=1536)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "game_move_values_bench.json"))
    args = ap.parse_args()
    if args.part == "selfplay":
        args.games = 64 if args.games is None else args.games[0]
    elif args.games is None:
        args.games = [8, 64, 512]
    out = {part: "not measured" for part in PARTS}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0)
    t0 = time.perf_counter()
    out[args.part] = {"gate": part_gate, "playouts": part_playouts, "update": part_update, "selfplay": part_selfplay}[args.part](args)
    out[args.part]["wall_seconds"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""What a pair reply table per game costs (bkt_reply2_playouts_tables, bkt_reply2_update_tables), on one MI355X.
By tools/game_tables_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps, by HIP events; every
part is a process of its own.  Only the gate has a threshold; everything else is recorded.

    python tools/game_pair_tables_bench.py gate      [--games 8 64 512] [--reps 3]
    python tools/game_pair_tables_bench.py playouts  [--rows 4096 65536] [--reps 3]
    python tools/game_pair_tables_bench.py update    [--records 1536] [--playouts 64] [--reps 3]
    python tools/game_pair_tables_bench.py selfplay  [--games 64] [--rollouts 400] [--playouts 64] [--share-games 8]
    (each with [--out profiles/game_pair_tables_bench.json]: a part replaces its own entry of that file and leaves the others)

gate        G games x 3 records x 64 playouts, pair tables learned from a first batch.  New: one bkt_reply2_playouts_tables
            (one per 65,536 rows: two at 512 games) plus one bkt_reply2_update_tables.  Baseline, what the library offered
            before: G bkt_reply2_playouts plus G bkt_reply2_update, one pair per game, on one stream.  Both leave the same
            tables (checked).  ratio = baseline / new must be >= 1.0 at 64 games; 8 and 512 are reported.
playouts    bkt_reply2_playouts_tables with tables=1 and with 64 copies of one learned table (slot = row % 64) against
            bkt_reply2_playouts with that table, at every size of --rows: the price of reading the pair byte from global
            memory instead of LDS.
update      bkt_reply2_update_tables with 1, 64 and 512 tables (slot = record % tables) against bkt_reply2_update and against
            bkt_reply_update_tables (single-move tables, the same counts), on --records x --playouts real histories.
selfplay    --games games x --rollouts rollouts, playout_value --playouts, playout_prior 1: plain on the Python loop, rave=4
            with a single-move table per game, rave=4 with a pair table per game.  Seconds, games/min, mean game length,
            black/white wins, the tables' occupancy at the end; the shares of playout plies that pairs and singles decided
            from one more run of --share-games games, not timed.
No strength figure of the pool engine is measured here.  A part that did not run reads "not measured".
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

from bokego_amd import _trainlib as T  # noqa: E402
from bokego_amd import go, replies, rollout, selfplay  # noqa: E402
from bokego_amd import lockstep as L  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
PARTS = ("gate", "playouts", "update", "selfplay")
DEV = torch.device("cuda", 0)
CAP = rollout.MAX_PLIES
SHAPE = (2, 82, 81)


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _best(paths, reps, before=lambda: None):
    """Warm-up, then the paths alternated, best of reps; before() runs ahead of every timed call, outside the clock."""
    for fn in paths.values():
        before()
        fn()
    best = {}
    for _ in range(reps):
        for name, fn in paths.items():
            before()
            torch.cuda.synchronize()
            ms, _ = _event_ms(fn)
            best[name] = min(ms, best.get(name, ms))
    return best


def golden_records(n):
    """n position records: the mid-game golden positions, cycled."""
    pos = json.load(open(os.path.join(GOLDEN, "positions.json")))["positions"][20:]
    recs = np.stack([np.frombuffer(bytes(go.Game(board=r["board"], ko=r["ko"], last_move=r["last_move"], turn=r["turn"])._pos),
                                   np.uint8) for r in pos[:min(n, len(pos))]])
    return np.ascontiguousarray(recs[np.arange(n) % len(recs)])


def _chunks(rows):
    return range(0, rows, T.MAX_BATCH)


def _won(pos, recs, n):
    score = torch.cat([T.area_score(pos[s:s + T.MAX_BATCH], L.KOMI) for s in _chunks(len(pos))])
    return ((score > 0).view(len(recs), n) == L.black_to_move(recs)[:, None]).reshape(-1).to(torch.uint8)


def _empty(count=None):
    return torch.full(SHAPE if count is None else (count,) + SHAPE, replies.NONE, dtype=torch.uint8, device=DEV)


def bench_gate(games, n, reps, seed):
    R = 3 * games
    recs = torch.from_numpy(golden_records(R)).to(DEV)
    start = recs.repeat_interleave(n, 0)
    ctr = L.value_counters_device(recs, n)
    slots = (torch.arange(R, device=DEV, dtype=torch.int32) // 3).contiguous()
    row_slots = slots.repeat_interleave(n).contiguous()
    learned = _empty(games)

    def play_all(tables, pos, key):
        return torch.cat([T.reply2_playouts(pos[s:s + T.MAX_BATCH], key, ctr[s:s + T.MAX_BATCH], None, None, tables, CAP,
                                            slots=row_slots[s:s + T.MAX_BATCH])[2] for s in _chunks(len(pos))])

    pos = start.clone()                                               # the first batch: scored, folded into the tables
    moves = play_all(learned, pos, seed)
    T.reply2_update(recs, moves, _won(pos, recs, n), R, n, learned, slots=slots)
    pos = start.clone()                                               # who wins the timed batch (its playouts are fixed by the tables)
    play_all(learned, pos, seed + 1)
    won = _won(pos, recs, n)
    many = torch.empty((T.load().bkt_reply2_tables_scratch_bytes(games),), dtype=torch.uint8, device=DEV)
    single = torch.empty((T.load().bkt_reply2_scratch_bytes(),), dtype=torch.uint8, device=DEV)
    tables, work = learned.clone(), start.clone()

    def reset():
        tables.copy_(learned)
        work.copy_(start)

    def new():
        T.reply2_update(recs, play_all(tables, work, seed + 1), won, R, n, tables, many, slots=slots)

    def baseline():
        for g in range(games):
            r, w = slice(3 * g, 3 * g + 3), slice(3 * n * g, 3 * n * (g + 1))
            m = T.reply2_playouts(work[w], seed + 1, ctr[w], None, None, tables[g], CAP)[2]
            T.reply2_update(recs[r], m, won[w], 3, n, tables[g], single)

    after = {}
    for name, fn in (("new", new), ("baseline", baseline)):            # the same tables either way
        reset()
        fn()
        after[name] = tables.clone()
    assert torch.equal(after["new"], after["baseline"]) and not torch.equal(after["new"], learned)
    best = _best({"new": new, "baseline": baseline}, reps, reset)
    return {"games": games, "records": R, "playouts": n, "rows": R * n, "playout_launches_new": len(_chunks(R * n)),
            "pair_occupancy_mean": float((learned[:, :, :81] <= 80).sum((1, 2, 3)).float().mean()),
            "single_occupancy_mean": float((learned[:, :, 81] <= 80).sum((1, 2)).float().mean()), "new_ms": best["new"],
            "baseline_ms": best["baseline"], "ratio": best["baseline"] / best["new"]}


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


def _learned_table(recs, n, seed):
    table = _empty()
    pos = recs.repeat_interleave(n, 0)
    moves = T.reply2_playouts(pos, seed, L.value_counters_device(recs, n), None, None, table, CAP)[2]
    T.reply2_update(recs, moves, _won(pos, recs, n), len(recs), n, table)
    return table


def part_playouts(args):
    out = {}
    for rows in args.rows:
        start = torch.from_numpy(golden_records(rows)).to(DEV)
        ctr = L.counters_to_device(rollout.default_counters(rows, rollout.record_turns(start.cpu().numpy())), rows, DEV)
        table = _learned_table(start[:64].contiguous(), 16, args.seed)
        none = _empty()
        one, many = table[None].contiguous(), table[None].repeat(64, 1, 1, 1).contiguous()
        zero = torch.zeros((rows,), dtype=torch.int32, device=DEV)
        spread = (torch.arange(rows, device=DEV, dtype=torch.int32) % 64).contiguous()
        paths = {"single": lambda: T.reply2_playouts(start.clone(), args.seed, ctr, None, None, table, CAP),
                 "tables_1": lambda: T.reply2_playouts(start.clone(), args.seed, ctr, None, None, one, CAP, slots=zero),
                 "tables_64": lambda: T.reply2_playouts(start.clone(), args.seed, ctr, None, None, many, CAP, slots=spread),
                 "single_all_255": lambda: T.reply2_playouts(start.clone(), args.seed, ctr, None, None, none, CAP),
                 "tables_1_all_255": lambda: T.reply2_playouts(start.clone(), args.seed, ctr, None, None, none[None], CAP, slots=zero)}
        want = paths["single"]()
        for name in ("tables_1", "tables_64"):                        # the same games
            assert all(torch.equal(a, b) for a, b in zip(paths[name](), want))
        best = _best(paths, args.reps)
        out[str(rows)] = r = {"rows": rows, "pair_occupancy": int((table[:, :81] <= 80).sum()),
                              "single_occupancy": int((table[:, 81] <= 80).sum()), **{f"{k}_ms": v for k, v in best.items()},
                              "ratio_tables_1": best["tables_1"] / best["single"], "ratio_tables_64": best["tables_64"] / best["single"],
                              "ratio_all_255": best["tables_1_all_255"] / best["single_all_255"]}
        print(f"{rows} rows: bkt_reply2_playouts {best['single']:.3f} ms, tables=1 x{r['ratio_tables_1']:.3f}, 64 copies "
              f"x{r['ratio_tables_64']:.3f}; all-255 tables {best['single_all_255']:.3f} ms, tables=1 x{r['ratio_all_255']:.3f}", flush=True)
    return out


def part_update(args):
    R, n = args.records, args.playouts
    recs = torch.from_numpy(golden_records(R)).to(DEV)
    pos = recs.repeat_interleave(n, 0)
    moves = torch.cat([T.random_playouts(pos[s:s + T.MAX_BATCH], args.seed, L.value_counters_device(recs, n)[s:s + T.MAX_BATCH],
                                         CAP)[2] for s in _chunks(R * n)])
    won = _won(pos, recs, n)
    one = _empty()
    scratch1 = torch.empty((T.load().bkt_reply2_scratch_bytes(),), dtype=torch.uint8, device=DEV)
    scratch_s = torch.empty((T.load().bkt_reply_scratch_bytes(R),), dtype=torch.uint8, device=DEV)
    paths = {"pair_single": lambda: T.reply2_update(recs, moves, won, R, n, one, scratch1)}
    for count in (1, 64, 512):
        tables = _empty(count)
        singles = torch.full((count, 2, 81), replies.NONE, dtype=torch.uint8, device=DEV)
        slots = (torch.arange(R, device=DEV, dtype=torch.int32) % count).contiguous()
        scratch = torch.empty((T.load().bkt_reply2_tables_scratch_bytes(count),), dtype=torch.uint8, device=DEV)
        paths[f"pair_tables_{count}"] = (lambda t=tables, s=slots, x=scratch: T.reply2_update(recs, moves, won, R, n, t, x, slots=s))
        paths[f"single_tables_{count}"] = (lambda t=singles, s=slots: T.reply_update_tables(recs, moves, won, R, n, t, s, scratch_s))
    best = _best(paths, args.reps)
    out = {"records": R, "playouts": n, "max_plies": CAP, **{f"{name}_ms": ms for name, ms in best.items()}}
    print(f"{R} x {n} histories: bkt_reply2_update {best['pair_single']:.4f} ms; bkt_reply2_update_tables 1 / 64 / 512: "
          f"{best['pair_tables_1']:.4f} / {best['pair_tables_64']:.4f} / {best['pair_tables_512']:.4f} ms; bkt_reply_update_tables: "
          f"{best['single_tables_1']:.4f} / {best['single_tables_64']:.4f} / {best['single_tables_512']:.4f} ms", flush=True)
    return out


def part_selfplay(args):
    base = dict(prior=1.0, seed=args.seed)
    kw = dict(n_games=args.games, rollouts=args.rollouts)
    kinds = {"plain_python_loop": (dict(), dict(native_loop=False)),
             "game_rave_replies": (dict(rave=True, replies=True, games=args.games), dict(rave=4.0)),
             "game_rave_reply_pairs": (dict(rave=True, pair_games=args.games), dict(rave=4.0))}
    selfplay.self_play(rollout.PlayoutEvaluator(None, args.playouts, **base), n_games=2, rollouts=8, max_turns=4)     # warm-up
    out = {"games": args.games, "rollouts": args.rollouts, "playouts": args.playouts}
    for name, (ev_kw, sp_kw) in kinds.items():
        ev = rollout.PlayoutEvaluator(None, args.playouts, **base, **ev_kw)
        torch.cuda.synchronize()
        local, total = selfplay.self_play(ev, **kw, **sp_kw)
        out[name] = r = {"seconds": local["seconds"], "games_per_min": args.games / local["seconds"] * 60,
                         "mean_game_length": total["plies"] / max(total["games"], 1), "black_wins": total["black_wins"],
                         "white_wins": total["white_wins"], "steps": local["steps"], "native_loop": local["native_loop"]}
        if ev.replies is not None:
            r["occupancy_mean"] = float(np.mean(ev.replies.occupancy()))
        if isinstance(ev.replies, replies.ReplyTables2):
            r["pair_occupancy_mean"] = float(np.mean(ev.replies.pairs_occupancy()))
        print(f"{name}: {r['seconds']:.1f} s, {r['games_per_min']:.1f} games/min, {r['mean_game_length']:.1f} plies/game, "
              f"B {r['black_wins']:.0f} : W {r['white_wins']:.0f}", flush=True)
    ev = rollout.PlayoutEvaluator(None, args.playouts, rave=True, pair_games=args.share_games, **base)
    seen, submit = {"plies": 0, "pair": 0, "single": 0}, ev.submit

    def counting(recs, n_policy, games=None):
        before = ev.replies.array.copy()
        h = submit(recs, n_policy, games=games)
        moves = rollout._numpy(h.run.moves)
        recs = np.ascontiguousarray(recs, np.uint8)
        seen["plies"] += int((np.cumsum(moves <= rollout.MOVE_NONE, 1) == 0).sum())
        for i, g in enumerate(games):                                 # the tables as they stood while the playouts ran
            p, s = replies.reply2_plies_of(before[g], recs[i:i + 1], moves[i * ev.playouts:(i + 1) * ev.playouts], ev.playouts)
            seen["pair"], seen["single"] = seen["pair"] + p, seen["single"] + s
        return h

    ev.submit = counting
    selfplay.self_play(ev, n_games=args.share_games, rollouts=args.rollouts, rave=4.0)
    plies = max(seen["plies"], 1)
    out["table_share"] = {"games": args.share_games, "plies": seen["plies"], "pair_plies": seen["pair"], "single_plies": seen["single"],
                          "pair_share": seen["pair"] / plies, "single_share": seen["single"] / plies,
                          "occupancy": ev.replies.occupancy().tolist(), "pair_occupancy": ev.replies.pairs_occupancy().tolist()}
    print(f"pairs decided {100 * seen['pair'] / plies:.1f} % and singles {100 * seen['single'] / plies:.1f} % of {seen['plies']} "
          f"playout plies ({args.share_games} games, not timed)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS)
    ap.add_argument("--games", type=int, nargs="+", default=None, help="gate: the pool sizes (8 64 512); selfplay: the games (64)")
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--records", type=int, default=1536)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=400)
    ap.add_argument("--share-games", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "game_pair_tables_bench.json"))
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

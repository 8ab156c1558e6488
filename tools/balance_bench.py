"""What the gradient sums of simulation balancing cost in one launch (bkt_balance_sums), and what tables fitted
for the playout value do to that value, on one MI355X.  One figure has a threshold, the gate; the others are recorded.
tools/mm_fit_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps by HIP events, every part a
process of its own under its own time limit.

    python tools/balance_bench.py launch   [--rows 4096 65536] [--reps 3]
    python tools/balance_bench.py gate     [--positions 64] [--samples 64] [--reps 3]
    python tools/balance_bench.py gradient [--positions 4096] [--reps 3]
    python tools/balance_bench.py quality  [--fit-games 4096] [--quality-games 4096] [--iterations 20] [--lr 1 ...]
    (each with [--out profiles/balance_bench.json]: a part replaces its own entry of that file and leaves the others)

launch   _trainlib.balance_sums against _trainlib.tactical_playouts on the same rows (ply-40 records of policy_19 games,
         repeated to --rows; a seeded pair of tables; coefficients over +-128): the ratio is the price of the booking.  No
         threshold.
gate     the gradient sums of --positions positions x --samples playouts: one balance launch, against the same integers by
         the lock-step route -- mmfit.pack of the recorded histories of the same playouts (not timed: the baseline is given
         them), then torch gathers, an integer floor division and integer index_add_ on the packed words.  `ratio` =
         baseline / ours must be >= 1.0.  The two results are compared for equality.
gradient one balance.gradient() over --positions positions at M = N = 64: three launches per 1,024 positions.
quality  positions at ply 40 of --fit-games policy_19 games (seed --fit-seed), labelled with the finished game's winner;
         balance.fit from the neutral pair and from the MM pair (mmfit.fit, 20 iterations) at every --lr; on the ply-40
         positions of --quality-games other games (seed --quality-seed): the error and the sign agreement of the N = 64
         value for no tables, the sequential pair, the MM pair, and the balanced pairs after every iteration (fit's log);
         the move-prediction log-likelihood of the final balanced pairs (mmfit.evaluate); the seconds of a whole fit.
A part that did not run reads "not measured".
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bokego_amd import _trainlib as T  # noqa: E402
from bokego_amd import balance, mmfit, patterns, rollout, tactics  # noqa: E402
from bokego_amd import lockstep as L  # noqa: E402
from mm_fit_bench import _engine, _event_ms, sequential_pair  # noqa: E402
from pattern_playout_bench import QUALITY_PLY, _timed, policy_games  # noqa: E402

PARTS = ("launch", "gate", "gradient", "quality", "match")
GATE_RATIO = 1.0
Q = balance.Q


def _positions(games, seed, ply=QUALITY_PLY):
    """(positions, targets, start, fin) of `games` policy_19 games."""
    eng = _engine(games)
    try:
        start, fin = policy_games(eng, games, seed)
    finally:
        eng.close()
    pos, tgt, _, _ = balance.labelled_positions(start, fin.moves, plies=(ply,))
    return pos, tgt, start, fin


def _seeded_pair():
    rng = np.random.default_rng(29)
    return (patterns.PatternTable(rng.integers(16, 4096, patterns.ENTRIES).astype(np.uint16)),
            tactics.TacticTable(rng.integers(64, 1024, tactics.ENTRIES).astype(np.uint16)))


def _best(paths, reps, label):
    best, last = {}, {}
    for fn in paths.values():
        fn()                                                            # warm-up
    for rep in range(reps):                                             # alternated
        for name, fn in paths.items():
            ms = _event_ms(lambda: last.__setitem__(name, fn()))
            best[name] = min(ms, best.get(name, ms))
            print(f"  {label}, run {rep}: {name} {ms:.3f} ms", flush=True)
    return best, last


def part_launch(args):
    pos0, _, _, _ = _positions(1024, args.fit_seed)
    table, tac = _seeded_pair()
    dev = torch.device("cuda", 0)
    p, t = table.device(dev), tac.device(dev)
    out = {"max_plies": rollout.MAX_PLIES, "reps": args.reps}
    for rows in args.rows:
        recs = torch.from_numpy(pos0[np.arange(rows) % len(pos0)]).to(dev)
        ctr = torch.from_numpy(L.game_counters(np.arange(rows, dtype=np.uint64), 0, 5)).to(dev)
        coef = torch.from_numpy(np.random.default_rng(1).integers(-128, 129, rows)).to(dev)
        paths = {"balance": lambda: T.balance_sums(recs.clone(), 7, ctr, p, t, coef, rollout.MAX_PLIES, history=False),
                 "tactical": lambda: T.tactical_playouts(recs.clone(), 7, ctr, p, t, rollout.MAX_PLIES, history=False)}
        best, last = _best(paths, args.reps, f"{rows} rows")
        assert torch.equal(last["balance"][3], last["tactical"][1])     # the same games
        out[f"rows={rows}"] = {"balance_ms": best["balance"], "tactical_ms": best["tactical"], "ratio": best["balance"] / best["tactical"],
                               "plies": int(last["tactical"][1].sum())}
        print(f"{rows} rows: balance {best['balance']:.3f} ms, tactical {best['tactical']:.3f} ms, x{best['balance'] / best['tactical']:.2f}", flush=True)
    return out


def lockstep_sums(start, hist, coef, table, tac):
    """The sums of bkt_balance_sums by the route there was before it: start uint8 [G,192] and hist int16 [G,L] on the device,
    the recorded playouts; coef int64 [G]; table, tac the device tables (int16 bits) -> (grad_p, grad_t) int64."""
    data = mmfit.pack(start, hist.cpu().numpy())                        # codes int32 [R,81], moves int32 [R]: ply-major
    live = (hist > T.MOVE_NONE).t()                                     # [L,G]
    c = coef[None, :].expand(live.shape)[live]                          # the coefficient of every packed row
    codes, mv = data.codes, data.moves.to(torch.int64)
    ok = codes < 0
    idx, code = (codes & 0x1FFFF).to(torch.int64), ((codes >> 17) & 63).to(torch.int64)
    P = (table.to(torch.int64) & 0xFFFF)[idx].clamp(min=1)
    w = ((P * (tac.to(torch.int64) & 0xFFFF)[code]) >> 8).clamp(min=1) * ok
    S = w.sum(1)
    d = -torch.div(w << Q, S.clamp(min=1)[:, None], rounding_mode="floor")
    rows = torch.nonzero((mv >= 0) & (S > 0))[:, 0]
    d[rows, mv[rows]] += 1 << Q
    value = c[:, None] * d
    grad_p = torch.zeros(T.PATTERN_ENTRIES, dtype=torch.int64, device=codes.device).index_add_(0, idx[ok], value[ok])
    grad_t = torch.zeros(T.TACTIC_ENTRIES, dtype=torch.int64, device=codes.device).index_add_(0, code[ok], value[ok])
    return grad_p, grad_t


def part_gate(args):
    pos0, _, _, _ = _positions(max(args.positions, 64), args.fit_seed)
    table, tac = _seeded_pair()
    dev = torch.device("cuda", 0)
    p, t = table.device(dev), tac.device(dev)
    part = torch.from_numpy(pos0[:args.positions]).to(dev)
    recs = part.repeat_interleave(args.samples, 0)
    ctr = L.value_counters_device(part, args.samples)
    coef = torch.from_numpy(np.random.default_rng(2).integers(-128, 129, len(recs))).to(dev)
    hist = T.tactical_playouts(recs.clone(), 7, ctr, p, t, rollout.MAX_PLIES)[2]        # the recorded playouts, not timed
    hist = hist[:, :int((hist > T.MOVE_NONE).sum(1).max())].contiguous()
    paths = {"ours": lambda: T.balance_sums(recs.clone(), 7, ctr, p, t, coef, rollout.MAX_PLIES, history=False)[:2],
             "baseline": lambda: lockstep_sums(recs, hist, coef, p, t)}
    best, last = _best(paths, args.reps, f"{args.positions} x {args.samples}")
    assert torch.equal(last["ours"][0], last["baseline"][0]) and torch.equal(last["ours"][1], last["baseline"][1])
    ratio = best["baseline"] / best["ours"]
    print(f"{args.positions} positions x {args.samples} playouts, {int((hist > T.MOVE_NONE).sum())} plies: ours {best['ours']:.3f} ms, "
          f"lock-step baseline {best['baseline']:.3f} ms, x{ratio:.2f} ({'passes' if ratio >= GATE_RATIO else 'FAILS'} the gate of {GATE_RATIO})", flush=True)
    return {"gate": GATE_RATIO, "positions": args.positions, "samples": args.samples, "plies": int((hist > T.MOVE_NONE).sum()),
            "ours_ms": best["ours"], "baseline_ms": best["baseline"], "ratio": ratio, "passes": bool(ratio >= GATE_RATIO),
            "equal_integers": True, "reps": args.reps}


def part_gradient(args):
    pos, tgt, _, _ = _positions(args.positions, args.fit_seed)
    table, tac = _seeded_pair()
    balance.gradient(pos[:64], tgt[:64], table, tac, 64, 64, 1)           # warm-up
    best = None
    for rep in range(args.reps):
        g, dt = _timed(lambda: balance.gradient(pos, tgt, table, tac, 64, 64, 1))
        best = dt if best is None else min(best, dt)
        print(f"  gradient over {len(pos)} positions, run {rep}: {dt:.3f} s", flush=True)
    return {"positions": int(len(pos)), "M": 64, "N": 64, "seconds": best, "mse": g.mse, "reps": args.reps}


def part_quality(args):
    pos, tgt, fit_start, fit_fin = _positions(args.fit_games, args.fit_seed)
    q_pos, q_tgt, q_start, q_fin = _positions(args.quality_games, args.quality_seed)
    mm = mmfit.fit(mmfit.pack(fit_start, fit_fin.moves), 20, 1.0)
    pairs = {"no_tables": (None, None), "sequential_pair": sequential_pair(fit_start, fit_fin.moves), "mm_pair": mmfit.tables(mm.gp, mm.gt)}
    out = {"fit": {"games": args.fit_games, "seed": args.fit_seed, "positions": int(len(pos))},
           "test": {"games": args.quality_games, "seed": args.quality_seed, "positions": int(len(q_pos))},
           "ply": QUALITY_PLY, "M": 64, "N": 64, "iterations": args.iterations, "value_seed": args.seed}
    n = len(q_pos)
    for name, (p, t) in pairs.items():
        out[name] = dict(balance.value_error(q_pos, q_tgt, p, t, 64, args.seed),
                         ply_40_moves=mmfit.evaluate(q_start, q_fin.moves, p, t, plies=[QUALITY_PLY]))
        print(f"{name}: mse {out[name]['mse']:.4f}, agreement {out[name]['agreement']:.4f} (standard error "
              f"{np.sqrt(out[name]['agreement'] * (1 - out[name]['agreement']) / n):.4f}), ply-40 ll {out[name]['ply_40_moves']['mean_ll']:.4f}", flush=True)
    for start_name, start in (("neutral", None), ("mm", (mm.gp, mm.gt))):
        for lr in args.lr:
            f, dt = _timed(lambda: balance.fit(pos, tgt, args.iterations, lr, 64, 64, start, seed=args.seed + 1000,
                                               held_out=(q_pos, q_tgt)))
            row = {"fit_seconds": dt, "log": f.log, "gt": f.gt.tolist(), "gp_min": int(f.gp.min()), "gp_max": int(f.gp.max()),
                   "ply_40_moves": mmfit.evaluate(q_start, q_fin.moves, f.patterns, f.tactics, plies=[QUALITY_PLY]),
                   "final": balance.value_error(q_pos, q_tgt, f.patterns, f.tactics, 64, args.seed)}
            out[f"balanced_from_{start_name}_lr={lr:g}"] = row
            print(f"from {start_name}, lr {lr:g} ({dt:.1f} s): " + "; ".join(
                f"it {r['iteration']} train {r['mse'] if r['mse'] is None else round(r['mse'], 4)} held-out {r['held_out_mse']:.4f} / "
                f"{r['held_out_agreement']:.4f}" for r in f.log if r["iteration"] in (0, 1, 5, 10, 20, args.iterations))
                + f"; ply-40 ll {row['ply_40_moves']['mean_ll']:.4f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS[:4])
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--positions", type=int, default=None)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fit-games", type=int, default=4096)
    ap.add_argument("--fit-seed", type=int, default=101)
    ap.add_argument("--quality-games", type=int, default=4096)
    ap.add_argument("--quality-seed", type=int, default=202)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--lr", type=float, nargs="+", default=[1.0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "balance_bench.json"))
    args = ap.parse_args()
    if args.positions is None:
        args.positions = 64 if args.part == "gate" else 4096
    out = {p: "not measured" for p in PARTS}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0)
    out[args.part] = {"launch": part_launch, "gate": part_gate, "gradient": part_gradient, "quality": part_quality}[args.part](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

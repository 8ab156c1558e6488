"""What one MM pass in one launch costs (bkt_mm_sums), what the jointly fitted tables predict on games they have
not seen, and what they do to the playout value, on one MI355X.  One figure has a threshold, the gate; the others are
recorded.  tools/pattern_prior_bench.py's protocol: a warm-up, the paths alternated in one process, best of --reps by HIP
events, every part a process of its own under its own time limit.

    python tools/mm_fit_bench.py gate    [--games 64 4096] [--reps 3]
    python tools/mm_fit_bench.py quality [--fit-games 4096] [--quality-games 4096]
    python tools/mm_fit_bench.py value   [--fit-games 4096] [--quality-games 4096] [--playouts 64] [--iterations 20]
    (each with [--out profiles/mm_fit_bench.json]: a part replaces its own entry of that file and leaves the others)

gate     one pass over the packed plies of --games policy_19 games (seed --fit-seed): bokego_amd._trainlib.mm_sums, one
         launch per 16,384 rows, against the same sums, totals and ranks from torch operations on the device over the same
         packed codes -- gathers, a float64 product, row sums, and torch.bincount with float64 weights, as tactics.counts
         does -- in one piece over all rows.  Strengths: random over a factor of 16 around 1.  `ratio` = torch / fused at
         4,096 games must be >= 1.0: the fused pass has no reason to exist if it is slower than what it replaces.  Also the
         pack time.  A torch pass that takes more than --slow-seconds is timed once, not --reps times: its bincount over
         131,072 bins adds float64 with atomics on a few hot addresses.
quality  fit on --fit-games policy_19 games (seed --fit-seed), test on --quality-games others (seed --quality-seed), at ply 40
         and over all plies: mean log-likelihood and top-1 / top-5 of the move played under mmfit.evaluate -- the draw's own
         weights, from bkt_move_weights -- for no tables, the sequential patterns table alone, the sequential pair
         (patterns.fit, tactics.fit on top) and the MM pair after 1, 2, 5, 10 and 20 iterations; the MM strengths before the
         rounding to uint16 (a pass over the test plies), and at --scales; the training set's penalised log-likelihood per
         half-iteration, and the training likelihood of the sequential pair beside the MM pair's.
value    DESIGN 18's measurement: the share of ply-40 positions where the sign of playout_value at N = --playouts agrees with
         the winner of the finished game, with the sequential pair and with the MM pair, and the seconds of that call.
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
from bokego_amd import lockstep as L  # noqa: E402
from bokego_amd import mmfit, patterns, reinforce, rollout, tactics  # noqa: E402
from bokego_amd.train import load_weights  # noqa: E402
from pattern_playout_bench import GOLDEN, QUALITY_PLY, _timed, policy_games  # noqa: E402

PARTS = ("gate", "quality", "value", "match")
GATE_RATIO, GATE_GAMES = 1.0, 4096
ITERATIONS = (1, 2, 5, 10, 20)


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _engine(games):
    return reinforce.policy_engine(load_weights(os.path.join(GOLDEN, "policy_19.bkw")), 0, min(max(games, 1), 4096))


def torch_sums(codes, moves, gp, gt):
    """bkt_mm_sums' results from torch operations, float64: codes int32 [R,81] and moves int32 [R] on the device, gp and gt
    float64 gamma tables on the device -> (den_p, den_t, total, chosen, rank)."""
    ok = codes < 0                                                      # bit 31
    idx, code = (codes & 0x1FFFF).to(torch.int64), ((codes >> 17) & 63).to(torch.int64)
    a, b = gp[idx], gt[code]
    s = a * b * ok
    E = s.sum(1)
    at = moves.clamp(0, 80).to(torch.int64)[:, None]
    s_m = torch.where((moves >= 0) & ok.gather(1, at)[:, 0], s.gather(1, at)[:, 0], torch.zeros_like(E))
    valid = s_m > 0
    point = torch.arange(81, device=codes.device)[None, :]
    rank = (ok & ((s > s_m[:, None]) | ((s == s_m[:, None]) & (point < moves[:, None])))).sum(1)
    rank = torch.where(valid, rank, torch.full_like(rank, -1))
    adds = ok & valid[:, None]
    inv = (1.0 / E.clamp(min=1e-300))[:, None]
    den_p = torch.bincount(idx[adds], weights=(b * inv)[adds], minlength=T.PATTERN_ENTRIES)
    den_t = torch.bincount(code[adds], weights=(a * inv)[adds], minlength=T.TACTIC_ENTRIES)
    return den_p, den_t, E, s_m, rank


def part_gate(args):
    eng = _engine(max(args.games))
    out = {"gate": GATE_RATIO, "reps": args.reps}
    try:
        for games in args.games:
            start, fin = policy_games(eng, games, args.fit_seed)
            for _ in range(2):                                          # the first packs the warm-up
                data, t_pack = _timed(lambda: mmfit.pack(start, fin.moves))
            rng = np.random.default_rng(28)
            gp = (65536 * 2.0 ** rng.uniform(-2, 2, T.PATTERN_ENTRIES)).astype(np.int64)
            gt = (65536 * 2.0 ** rng.uniform(-2, 2, T.TACTIC_ENTRIES)).astype(np.int64)
            gp_d, gt_d = torch.from_numpy(gp).cuda(), torch.from_numpy(gt).cuda()
            fp, ft = gp_d.to(torch.float64) / 65536, gt_d.to(torch.float64) / 65536      # made once, outside the timing
            paths = {"fused": lambda: T.mm_sums(data.codes, data.moves, gp_d, gt_d),
                     "torch": lambda: torch_sums(data.codes, data.moves, fp, ft)}
            paths["fused"]()                                            # warm-up
            torch_sums(data.codes[:256], data.moves[:256], fp, ft)      # (of the torch path on a few rows: a pass of it over
            best, last, slow = {}, {}, False                            # all rows can take a minute)
            for rep in range(args.reps):                                # alternated
                for name, fn in paths.items():
                    if name == "torch" and slow:
                        continue                                        # a run above --slow-seconds is not repeated
                    ms = _event_ms(lambda: last.__setitem__(name, fn()))
                    best[name] = min(ms, best.get(name, ms))
                    slow = slow or (name == "torch" and ms > 1e3 * args.slow_seconds)
                    print(f"  {games} games, run {rep}: {name} {ms:.3f} ms", flush=True)
            a, b = last["fused"], last["torch"]                       # the same sums
            assert torch.equal(a[4].to(torch.int64) >= 0, b[4] >= 0)
            for x, y, unit in ((a[0], b[0], 2.0 ** 32), (a[1], b[1], 2.0 ** 32), (a[2], b[2], 65536.0)):
                err = ((x.to(torch.float64) / unit - y).abs() / y.abs().clamp(min=1.0)).max().item()
                assert err < 1e-3, err
            r = {"games": games, "rows": int(len(data.moves)), "moves": int(data.played_t.sum()), "pack_seconds": t_pack,
                 "fused_ms": best["fused"], "torch_ms": best["torch"], "ratio": best["torch"] / best["fused"]}
            if games == GATE_GAMES:
                r["passes"] = bool(r["ratio"] >= GATE_RATIO)
            out[f"games={games}"] = r
            print(f"{games} games, {r['rows']} plies: pack {t_pack:.3f} s; one pass fused {r['fused_ms']:.3f} ms, torch "
                  f"{r['torch_ms']:.3f} ms, x{r['ratio']:.2f}" + (f" ({'passes' if r['passes'] else 'FAILS'} the gate of "
                                                                    f"{GATE_RATIO})" if "passes" in r else ""), flush=True)
    finally:
        eng.close()
    return out


def sequential_pair(start, moves):
    table = patterns.PatternTable(patterns.weights(*patterns.symmetrise(*patterns.counts(start, moves))))
    return table, tactics.TacticTable(tactics.weights(*tactics.counts(start, moves, table)))


def _both(start, moves, table, tac):
    return {"all_plies": mmfit.evaluate(start, moves, table, tac), "ply_40": mmfit.evaluate(start, moves, table, tac, plies=[QUALITY_PLY])}


def _games(args):
    eng = _engine(max(args.fit_games, args.quality_games))
    try:
        (fit_start, fit_fin), (q_start, q_fin) = (policy_games(eng, g, s) for g, s in ((args.fit_games, args.fit_seed),
                                                                                       (args.quality_games, args.quality_seed)))
    finally:
        eng.close()
    return fit_start, fit_fin, q_start, q_fin


def part_quality(args):
    fit_start, fit_fin, q_start, q_fin = _games(args)
    data, t_pack = _timed(lambda: mmfit.pack(fit_start, fit_fin.moves))
    test = mmfit.pack(q_start, q_fin.moves)
    seq_p, seq_t = sequential_pair(fit_start, fit_fin.moves)
    out = {"fit": {"games": args.fit_games, "seed": args.fit_seed, "rows": int(len(data.moves)), "pack_seconds": t_pack},
           "test": {"games": args.quality_games, "seed": args.quality_seed, "rows": int(len(test.moves))}, "prior": args.prior,
           "held_out": {"uniform": _both(q_start, q_fin.moves, None, None),
                        "sequential_patterns": _both(q_start, q_fin.moves, seq_p, None),
                        "sequential_pair": _both(q_start, q_fin.moves, seq_p, seq_t)},
           "training": {"sequential_pair": mmfit.evaluate(fit_start, fit_fin.moves, seq_p, seq_t)}}
    for k, v in out["held_out"].items():
        print(f"{k}: " + ", ".join(f"{w} ll {r['mean_ll']:.4f} top-1 {r['top1']:.4f} top-5 {r['top5']:.4f}" for w, r in v.items()), flush=True)
    for its in ITERATIONS:
        f, dt = _timed(lambda: mmfit.fit(data, its, args.prior))
        row = {"fit_seconds": dt}
        for scale in args.scales:
            row[f"scale={scale}"] = _both(q_start, q_fin.moves, *mmfit.tables(f.gp, f.gt, scale))
        s = mmfit.penalised((f.gp, f.gt), mmfit.sums(test, f.gp, f.gt), args.prior)
        row["before_rounding_all_plies"] = {k: s[k] for k in ("moves", "mean_ll", "top1", "top5")}
        out["held_out"][f"mm_{its}"] = row
        print(f"MM {its} iterations ({dt:.2f} s): before rounding ll {s['mean_ll']:.4f} top-1 {s['top1']:.4f} top-5 {s['top5']:.4f}; "
              + "; ".join(f"{k} all ll {v['all_plies']['mean_ll']:.4f} top-1 {v['all_plies']['top1']:.4f} top-5 "
                          f"{v['all_plies']['top5']:.4f}, ply 40 top-1 {v['ply_40']['top1']:.4f} top-5 {v['ply_40']['top5']:.4f}"
                          for k, v in row.items() if k.startswith("scale=")), flush=True)
    out["training"]["mm_log"] = [{k: row[k] for k in ("iteration", "penalised_ll", "mean_ll", "top1", "top5")} for row in f.log]
    out["training"]["mm_pair"] = {f"scale={scale}": mmfit.evaluate(fit_start, fit_fin.moves, *mmfit.tables(f.gp, f.gt, scale))
                                  for scale in args.scales}
    out["strengths"] = {"gt": f.gt.tolist(), "gp_min": int(f.gp.min()), "gp_max": int(f.gp.max()),
                        "gp_at_the_domain_edge": int(((f.gp == mmfit.G_MIN) | (f.gp == mmfit.G_MAX)).sum())}
    print("training mean ll: sequential pair", out["training"]["sequential_pair"]["mean_ll"], "MM pair",
          {k: v["mean_ll"] for k, v in out["training"]["mm_pair"].items()}, "MM strengths", f.log[-1]["mean_ll"], flush=True)
    return out


def part_value(args):
    fit_start, fit_fin, q_start, q_fin = _games(args)
    f = mmfit.fit(mmfit.pack(fit_start, fit_fin.moves), args.iterations, args.prior)
    pairs = {"sequential_pair": sequential_pair(fit_start, fit_fin.moves)}
    pairs.update({f"mm_pair_scale={scale}": mmfit.tables(f.gp, f.gt, scale) for scale in args.scales})
    rows = np.nonzero(q_fin.over & (q_fin.plies > QUALITY_PLY))[0]
    pos = torch.from_numpy(q_start[rows]).cuda()
    hist = torch.from_numpy(q_fin.moves[rows, :QUALITY_PLY].astype(np.int32)).cuda()
    status = torch.zeros(len(rows), dtype=torch.int32, device=pos.device)
    for k in range(QUALITY_PLY):
        status |= T.playout_step(pos, hist[:, k].contiguous(), None, None, None)
    assert not status.any().item()
    mover_wins = (torch.from_numpy(q_fin.score[rows] > 0).cuda() == L.black_to_move(pos)).cpu().numpy()
    out = {"ply": QUALITY_PLY, "positions": int(len(rows)), "playouts": args.playouts, "value_seed": args.seed,
           "iterations": args.iterations, "prior": args.prior}
    for fn in [lambda p=p, t=t: rollout.playout_value(pos, args.playouts, args.seed, patterns=p, tactics=t) for p, t in pairs.values()]:
        fn()                                                            # warm-up
    for name, (p, t) in pairs.items():
        best = None
        for _ in range(args.reps):
            v, dt = _timed(lambda: rollout.playout_value(pos, args.playouts, args.seed, patterns=p, tactics=t))
            best = dt if best is None else min(best, dt)
        out[name] = {"agreement": float(((v > 0) == mover_wins)[v != 0].sum() / len(rows)), "ties": float((v == 0).mean()),
                     "mean_abs_value": float(np.abs(v).mean()), "seconds": best}
        print(f"{name}: agreement {out[name]['agreement']:.4f}, {best:.3f} s", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=PARTS[:3])
    ap.add_argument("--games", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fit-games", type=int, default=4096)
    ap.add_argument("--fit-seed", type=int, default=101)
    ap.add_argument("--quality-games", type=int, default=4096)
    ap.add_argument("--quality-seed", type=int, default=202)
    ap.add_argument("--playouts", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--prior", type=float, default=1.0)
    ap.add_argument("--slow-seconds", type=float, default=5.0, help="gate: a torch pass slower than this is timed once")
    ap.add_argument("--scales", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mm_fit_bench.json"))
    args = ap.parse_args()
    out = {p: "not measured" for p in PARTS}
    if os.path.exists(args.out):
        out.update(json.load(open(args.out)))
    out["device"] = torch.cuda.get_device_name(0)
    out[args.part] = {"gate": part_gate, "quality": part_quality, "value": part_value}[args.part](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

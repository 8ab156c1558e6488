"""Simulation balancing: the playouts' two tables -- the 3x3 pattern weights (patterns.py) and the
tactical weights (tactics.py) -- fitted so that the playouts EVALUATE positions, not so that they imitate moves.

    python -m bokego_amd.balance fit -p POLICY [--games 4096] [--seed S] [--records DIR ...] [--plies 40] [--iterations 20]
                                     [--lr 1] [--playouts 64] [--samples 64] [--prior 0] [--scale 64]
                                     [--start-patterns P.npy --start-tactics T.npy] --patterns-out P.npy --tactics-out T.npy
    python -m bokego_amd.balance eval [--patterns P.npy] [--tactics T.npy] -p POLICY [--games N] [--seed S] [--plies 40]
                                      [--playouts 64]

The playouts draw a playable point in proportion to w = max(1, (P * T) >> 8): a log-linear policy whose parameters are
the log-strengths of the two tables.  patterns.fit + tactics.fit and mmfit fit them to predict moves; by DESIGN 18 and 28 a
better predictor is not a better evaluator.  Simulation balancing (Silver & Tesauro 2009; Huang, Coulom & Lin 2010)
descends on the squared error of the playout value itself: for a position r with target V*_r,

    V_r = the mean outcome of M playouts                       (rollout.playout_value)
    g_r = the mean over N further playouts of  z_j * sum_t psi(s_t, a_t),     psi = the gradient of log pi by theta
    theta += lr * (V*_r - V_r) * g_r

psi(s, a) for a feature is [the move carries it] minus the share of the draw of the candidates that carry it.  One launch
of bkt_balance_sums replays N playouts of every position and books exactly that, in integers (units of 2^-Q of a move),
times a signed integer coefficient per playout; sums_host is the same on the host rules, integer for integer.  gradient()
is three launches per batch of positions: (a) M playouts for D_r = round(V*_r M) - (2 wins_r - M), (b) N playouts under
another key, scored, for z_j = +-1, (c) the same N playouts again through bkt_balance_sums with coef_j = z_j D_r.  The
two sets are independent, as in Huang et al.; one set for both would be biased.  fit() takes plain gradient steps on
float64 log-strengths, pooled over the patterns' dihedral orbits as mmfit pools them, with weight decay towards the start as
the only regulariser, and plays every iteration with the tables as mmfit.tables() rounds them: the gradient is that of the
policy actually played.  The floats are computed on the host from integers that are the same on both rules, so a device
fit and a host fit end on the same bits.  No fitted table ships.
"""
import argparse
import collections

import numpy as np
import torch

from . import _trainlib as T
from . import lockstep as L
from . import mmfit as MM
from . import patterns as PT
from . import replay as RP
from . import rollout as RO
from . import tactics as TC

Q = T.BALANCE_Q
ONE = 1 << Q                                        # a whole move, in the units the sums are booked in
MAX_COEF = T.BALANCE_MAX_COEF
MAX_ROWS = T.BALANCE_MAX_ROWS                       # rows of one bkt_balance_sums launch
MAX_PLIES = RO.MAX_PLIES
KEY_STEP = 0x9E3779B97F4A7C15                       # gradient(): the key of the second playout set is the seed's plus this
POSITIONS_PER_BATCH = 1024                          # gradient(): positions per three launches

Sums = collections.namedtuple("Sums", "grad_p grad_t records over plies moves")
Sums.__doc__ = """What sums returns (numpy): grad_p int64 [patterns.ENTRIES], grad_t int64 [tactics.ENTRIES]; the final
records uint8 [B,192], over bool [B], plies int64 [B] and moves int16 [B,max_plies] of the games."""
Gradient = collections.namedtuple("Gradient", "grad_p grad_t norm mse D wins")
Gradient.__doc__ = """What gradient returns: grad_p, grad_t int64 (numpy), the sums of coef * d over all positions; norm =
M * N * R * 2^Q (a Python integer): grad / norm is the mean over positions of (V* - V) g; mse = mean((V* - V)^2), V = (2 wins
- M) / M; D int64 [R] and wins int64 [R] of launch (a)."""
Fit = collections.namedtuple("Fit", "gp gt patterns tactics log")

__all__ = ["Fit", "Gradient", "MAX_COEF", "MAX_ROWS", "ONE", "Q", "Sums", "coefficients", "fit", "gradient", "labelled_positions",
           "strengths_of_tables", "sums", "sums_host", "value_error"]


# ---- the sums -------------------------------------------------------------------------------------------------------------------
def _coef(coef, rows):
    c = np.asarray(coef)
    if c.shape != (rows,) or c.dtype.kind not in "iu":
        raise ValueError(f"coef must be integers [{rows}], got {c.dtype} {c.shape}")
    c = c.astype(np.int64)
    if rows and (c.min() < -MAX_COEF or c.max() > MAX_COEF):
        raise ValueError(f"coef: a coefficient is -{MAX_COEF}..{MAX_COEF}, got {c.min()}..{c.max()}")
    return c


def _max_plies(max_plies):
    max_plies = int(max_plies)
    if not 1 <= max_plies <= T.MAX_PLAYOUT_PLIES:
        raise ValueError(f"max_plies must be 1..{T.MAX_PLAYOUT_PLIES}, got {max_plies}")
    return max_plies


def _check_bound(rows, max_plies, coef):
    """The header's bound for sums added in int64: every entry stays below rows * max_plies * max|coef| * 2^(Q+1)."""
    top = int(np.abs(coef).max()) if len(coef) else 0
    if rows * max_plies * top * 2 * ONE >= 2 ** 63:
        raise ValueError(f"{rows} rows of {max_plies} plies with |coef| up to {top} could pass 2^63: split the rows")


def sums_host(recs, seed, counters, coef, patterns=None, tactics=None, max_plies=MAX_PLIES, over=None):
    """bkt_balance_sums in numpy, the definition (include/bokego_train.h says the same in words), on the host-rules playout
    loop of rollout.random_playouts(rules="host"): recs uint8 [B,192] (not modified), seed, counters int32 [B,4], coef
    integers [B] within MAX_COEF (else ValueError), patterns / tactics: as random_playouts, None for none; over: None or
    bool [B], rows that are left alone -> Sums.  At every ply of every row that is not over and has a playable point, with
    w_j the draw's weights, S their sum and m the point the draw picks, every playable j books coef * ((j == m) * 2^Q -
    floor(w_j 2^Q / S)) against its pattern index in grad_p and against its tactical code in grad_t."""
    RO._check_records(recs)
    recs = np.array(RO._numpy(recs), np.uint8, order="C")
    B, max_plies = len(recs), _max_plies(max_plies)
    coef = _coef(coef, B)
    _check_bound(B, max_plies, coef)
    table, tac = RO._table(patterns), RO._tactics(tactics)
    ctr = L.counters_to_host(counters, B)
    grad_p, grad_t = np.zeros(PT.ENTRIES, np.int64), np.zeros(TC.ENTRIES, np.int64)
    start_over = np.zeros(B, bool) if over is None else np.asarray(over).astype(bool)
    rows_of = np.nonzero(~start_over)[0]                              # _playout_host starts every row it is given

    def choose(k, part_all, live, ok, x0):
        part = part_all[live]
        index, code = PT.codes_host(part).astype(np.int64), TC.codes_host(part).astype(np.int64)
        t = np.full(ok.shape, TC.NEUTRAL, np.uint16) if tac is None else tac.entries(code)
        w = np.where(ok, TC.combine(None if table is None else table.entries(index), t), np.uint64(0)).astype(np.uint64)
        mv = PT.select_weighted(x0, w, ok)                             # w >= 1 on every playable point: the draw itself
        S = w.sum(1, dtype=np.uint64)
        c = coef[rows_of[live]]
        d = -((w << np.uint64(Q)) // np.maximum(S, np.uint64(1))[:, None]).astype(np.int64)
        picked = np.nonzero(mv >= 0)[0]
        d[picked, mv[picked]] += ONE
        books = ok & (c != 0)[:, None]                                 # a playable point has S > 0
        value = (c[:, None] * d)[books]
        MM._add_at(grad_p, index[books], value)
        MM._add_at(grad_t, code[books], value)
        return mv

    records, over_out = recs.copy(), start_over.copy()
    plies, moves = np.zeros(B, np.int64), np.full((B, max_plies), RO.MOVE_NONE, np.int16)
    if len(rows_of):
        fin = RO._playout_host(recs[rows_of], L.seed_u64(seed), ctr[rows_of], max_plies, L.KOMI, choose, "selected")
        records[rows_of], over_out[rows_of], plies[rows_of] = fin.records, fin.over, fin.plies
        moves[rows_of, :fin.moves.shape[-1]] = fin.moves
    return Sums(grad_p, grad_t, records, over_out, plies, moves)


def sums(recs, seed, counters, coef, patterns=None, tactics=None, max_plies=MAX_PLIES, rules="device", device=None, over=None):
    """The sums of a batch of playouts -> Sums (numpy).  rules="device": bkt_balance_sums, one launch per MAX_ROWS rows,
    into one accumulator (the bound that keeps it below 2^63 is checked first; ValueError otherwise: split the rows);
    rules="host": sums_host.  The arguments are sums_host's; recs, counters and coef may be tensors."""
    L.check_rules(rules)
    if rules == "host":
        return sums_host(recs, seed, RO._numpy(counters), RO._numpy(coef), patterns, tactics, max_plies, over)
    RO._check_records(recs)
    B, max_plies = len(recs), _max_plies(max_plies)
    table, tac = RO._table(patterns), RO._tactics(tactics)
    dev = RO._device(device, None, recs)
    pos = L.records_to_device(recs, dev, clone=True)
    ctr = L.counters_to_device(counters, B, dev, clone=False)
    c = T.balance_coef(coef if isinstance(coef, torch.Tensor) else _coef(coef, B), B, dev)
    _check_bound(B, max_plies, c.cpu().numpy())
    ov = None if over is None else torch.as_tensor(np.asarray(RO._numpy(over)).astype(np.uint8)).to(dev)
    gp, gt, ov, plies, moves, status = T.balance_sums(pos, L.seed_u64(seed), ctr, None if table is None else table.device(dev),
                                                      None if tac is None else tac.device(dev), c, max_plies, over=ov)
    RO._check_status(status, "selected")
    return Sums(gp.cpu().numpy(), gt.cpu().numpy(), pos.cpu().numpy(), ov.cpu().numpy() != 0,
                plies.cpu().numpy().astype(np.int64), moves.cpu().numpy())


# ---- the gradient ---------------------------------------------------------------------------------------------------------------
def _targets(targets, R):
    t = np.asarray(targets, np.float64)
    if t.shape != (R,) or not (np.abs(t) <= 1.0).all():               # (a NaN fails the comparison)
        raise ValueError(f"targets must be {R} numbers in [-1, 1]")
    return t


def _counts(M, N):
    M, N = RO._check_playouts(M), RO._check_playouts(N)
    if 2 * M > MAX_COEF:
        raise ValueError(f"M must be at most {MAX_COEF // 2}: |D| <= 2 M is a coefficient of bkt_balance_sums")
    return M, N


def coefficients(targets, wins, won, M):
    """(D int64 [R], coef int64 [R,N]) of gradient(): D_r = rint(V*_r M) - (2 wins_r - M) (numpy's rint: halves to even),
    coef[r, j] = +D_r where the side to move at position r won playout j of the second set, -D_r where it lost."""
    D = np.rint(np.asarray(targets, np.float64) * M).astype(np.int64) - (2 * np.asarray(wins, np.int64) - M)
    return D, np.where(np.asarray(won, bool), 1, -1).astype(np.int64) * D[:, None]


def gradient(positions, targets, patterns=None, tactics=None, M=64, N=64, seed=0, rules="device", device=None,
             max_plies=MAX_PLIES, komi=L.KOMI):
    """The simulation-balancing gradient of the tables (patterns, tactics: as random_playouts) at the positions uint8
    [R,192] with the targets float [R] in [-1, 1], from the side to move -> Gradient.  Per POSITIONS_PER_BATCH positions,
    three launches: (a) playout_value's M playouts under `seed` -> wins and D; (b) N playouts under the key seed +
    KEY_STEP (mod 2^64), scored -> who won each; (c) the same N playouts again through bkt_balance_sums (rules="host":
    sums_host) with coef = +-D.  The replay of (b) in (c) costs one playout launch more than a kernel that scored its own
    games would; it keeps scoring in the one place it lives.  The batches' integer sums are added on the host, in int64
    under the header's bound for all R * N rows (checked first)."""
    L.check_rules(rules)
    RO._check_records(positions)
    R = len(positions)
    targets, (M, N) = _targets(targets, R), _counts(M, N)
    max_plies = _max_plies(max_plies)
    if R * N * max_plies * 2 * M * 2 * ONE >= 2 ** 63:
        raise ValueError(f"{R} positions x {N} playouts of {max_plies} plies could pass 2^63 in int64: fewer positions a call")
    table, tac = RO._table(patterns), RO._tactics(tactics)
    key_a = L.seed_u64(seed)
    key_b = (key_a + KEY_STEP) & (2 ** 64 - 1)
    host = rules == "host"
    recs = np.array(RO._numpy(positions), np.uint8, order="C") if host else \
        L.records_to_device(positions, RO._device(device, None, positions), clone=False)
    grad_p, grad_t = np.zeros(PT.ENTRIES, np.int64), np.zeros(TC.ENTRIES, np.int64)
    wins_all, D_all = np.zeros(R, np.int64), np.zeros(R, np.int64)
    for s in range(0, R, POSITIONS_PER_BATCH):
        part = recs[s:s + POSITIONS_PER_BATCH]
        a = RO._playouts(part, M, key_a, rules, komi, table, tac, max_plies)
        b = RO._playouts(part, N, key_b, rules, komi, table, tac, max_plies)
        wins = np.asarray(RO._numpy(a.wins), np.int64)
        D, coef = coefficients(targets[s:s + len(part)], wins, RO._numpy(b.won), M)
        wins_all[s:s + len(part)], D_all[s:s + len(part)] = wins, D
        if host:
            c = sums_host(np.repeat(part, N, 0), key_b, RO.value_counters(part, N), coef.reshape(-1), table, tac, max_plies)
            gp, gt = c.grad_p, c.grad_t
        else:
            dev = part.device
            gp, gt, _, _, _, status = T.balance_sums(part.repeat_interleave(N, 0), key_b, L.value_counters_device(part, N),
                                                     None if table is None else table.device(dev),
                                                     None if tac is None else tac.device(dev), coef.reshape(-1), max_plies,
                                                     history=False)
            RO._check_status(status, "selected")
            gp, gt = gp.cpu().numpy(), gt.cpu().numpy()
        grad_p += gp
        grad_t += gt
    V = (2 * wins_all - M) / M
    return Gradient(grad_p, grad_t, M * N * R * ONE, float(np.mean((targets - V) ** 2)), D_all, wins_all)


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def strengths_of_tables(patterns=None, tactics=None, scale=64):
    """The strengths (gp, gt uint32, mmfit's fixed point: gamma = g / 65536) that mmfit.tables(gp, gt, scale) rounds back
    into the given tables -- what fit(start=) takes; None: gamma = 1 everywhere.  Clipped to mmfit's domain."""
    table, tac = RO._table(patterns), RO._tactics(tactics)
    gp = np.full(PT.ENTRIES, MM.G_ONE, np.int64) if table is None else \
        (2 * np.maximum(table.array.astype(np.int64), 1) * MM.G_ONE + scale) // (2 * scale)
    gt = np.full(TC.ENTRIES, MM.G_ONE, np.int64) if tac is None else \
        (2 * np.maximum(tac.array.astype(np.int64), 1) * MM.G_ONE + TC.NEUTRAL) // (2 * TC.NEUTRAL)
    return np.clip(gp, MM.G_MIN, MM.G_MAX).astype(np.uint32), np.clip(gt, MM.G_MIN, MM.G_MAX).astype(np.uint32)


def _strengths(theta):
    return np.clip(np.rint(np.exp(theta) * MM.G_ONE), MM.G_MIN, MM.G_MAX).astype(np.uint32)


def value_error(positions, targets, patterns=None, tactics=None, n=64, seed=0, rules="device", device=None):
    """How well the playout value of a pair of tables evaluates -> dict(positions, mse, agreement, ties): V =
    rollout.playout_value at n playouts; mse = mean((target - V)^2); agreement = the share of positions where V != 0 and
    its sign is the target's (a value of 0 agrees with nobody: DESIGN 18's yardstick); ties = the share with V == 0."""
    t = _targets(targets, len(positions))
    v = RO.playout_value(positions, n, seed, rules=rules, device=device, patterns=patterns, tactics=tactics).astype(np.float64)
    return dict(positions=len(t), mse=float(np.mean((t - v) ** 2)), agreement=float((((v > 0) == (t > 0)) & (v != 0)).mean()),
                ties=float((v == 0).mean()))



def fit(positions, targets, iterations=20, lr=1.0, M=64, N=64, start=None, prior=0.0, rules="device", seed=0, scale=64,
        held_out=None, device=None, max_plies=MAX_PLIES):
    """Simulation balancing -> Fit(gp, gt uint32 strengths, patterns PatternTable, tactics TacticTable, log).  theta, float64
    log-strengths of mmfit.GROUPS, start at `start` -- None: gamma = 1 everywhere, or a pair (gp, gt) of strengths, such as
    an mmfit.Fit's or strengths_of_tables(...).  Iteration i plays with mmfit.tables(strengths, scale) of the current theta
    under the seed `seed + i`, and steps

        theta += lr * pooled(grad) / norm - lr * prior * (theta - theta_start)

    pooled over the patterns' dihedral orbits (mmfit.pooled).  log[i], i = 0 .. iterations: "iteration", "mse" -- the
    training error gradient() measured with the tables the iteration played (None in the last row, whose tables no
    gradient was taken of) -- and with held_out=(positions, targets) "held_out_mse", "held_out_agreement" (value_error at M
    playouts).  The same arguments give the same bits on both rules."""
    L.check_rules(rules)
    iterations, lr, prior, scale = int(iterations), float(lr), float(prior), int(scale)
    if iterations < 0 or not 0.0 < lr < float("inf") or not 0.0 <= prior < float("inf"):
        raise ValueError("iterations must not be negative, lr must be positive and prior not negative")
    gp0, gt0 = strengths_of_tables() if start is None else (MM._strengths(g, group.entries, group.name).astype(np.uint32)
                                                            for g, group in zip(start, MM.GROUPS))
    theta0 = [np.log(g.astype(np.float64) / MM.G_ONE) for g in (gp0, gt0)]
    theta = [t.copy() for t in theta0]
    log = []
    for i in range(iterations + 1):
        g = [_strengths(t) for t in theta]
        table, tac = MM.tables(g[0], g[1], scale)
        row = dict(iteration=i, mse=None)
        if held_out is not None:
            e = value_error(held_out[0], held_out[1], table, tac, M, seed, rules, device)
            row.update(held_out_mse=e["mse"], held_out_agreement=e["agreement"])
        if i < iterations:
            grad = gradient(positions, targets, table, tac, M, N, L.seed_u64(seed + i), rules, device, max_plies)
            row["mse"] = grad.mse
            for k, (group, raw) in enumerate(zip(MM.GROUPS, (grad.grad_p, grad.grad_t))):
                step = MM.pooled(group, raw).astype(np.float64) / float(grad.norm)
                theta[k] = theta[k] + lr * step - lr * prior * (theta[k] - theta0[k])
        log.append(row)
    return Fit(g[0], g[1], table, tac, log)


# ---- the data -------------------------------------------------------------------------------------------------------------------
def labelled_positions(start_recs, moves, plies=(40,), komi=L.KOMI):
    """Positions out of finished games, labelled with the winner -> (positions uint8 [P,192], targets float64 [P] = +1 where
    the side to move at the position won the finished game, -1 where it lost, game int64 [P], ply int64 [P]).  start_recs
    uint8 [G,192] and moves [G,L] as patterns.counts takes them; the games are replayed on the host rules, a game gives
    its position before ply k for every k of `plies` it reaches, and its final record is scored by area (black wins a
    score > 0).  The label is noisy and unbiased for the games' own policy: DESIGN 18's and 28's yardstick."""
    start, moves = RP.check_games(start_recs, moves)
    want = sorted(set(int(k) for k in plies))
    if not want or want[0] < 0:
        raise ValueError("plies must name at least one ply, none negative")
    recs, taken = start, []           # one batch: recs is the walker's array of all games, and holds the final records at the end
    for k, _, live, recs, _, _ in RP.replay_host(start, moves, playable=False):
        if k in want:
            taken.append((recs[live].copy(), live, np.full(len(live), k, np.int64)))
    if not taken:
        return np.zeros((0, L.POS_BYTES), np.uint8), np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64)
    black_won = L.area_score_host(recs, komi) > 0
    positions = np.concatenate([p for p, _, _ in taken])
    game, ply = np.concatenate([g for _, g, _ in taken]), np.concatenate([k for _, _, k in taken])
    targets = np.where(black_won[game] == L.black_to_move(positions), 1.0, -1.0)
    return positions, targets, game, ply


# ---- the command line -----------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fit the playouts' pattern and tactics tables by simulation balancing, and "
                                             "measure the playout value of a pair")
    sub = ap.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="fit both tables on positions of policy games (and self-play records)")
    e = sub.add_parser("eval", help="the error and the sign agreement of the playout value of a pair of tables on fresh games")
    for p in (f, e):
        p.add_argument("-p", dest="p", metavar="POLICY", default=None, help="policy weights (.pt or .bkw)")
        p.add_argument("--seed", type=int, default=0 if p is f else 1)
        p.add_argument("--plies", type=int, nargs="+", default=[40], help="the plies positions are taken at")
        p.add_argument("--playouts", type=int, default=64, help="M: playouts of the value")
        p.add_argument("--device", type=int, default=0)
    f.add_argument("--games", type=int, default=4096, help="policy games from the empty board, played to the end")
    f.add_argument("--records", nargs="+", default=None, metavar="DIR", help="selfplay --out directories to add")
    f.add_argument("--iterations", type=int, default=20)
    f.add_argument("--lr", type=float, default=1.0, help="the step")
    f.add_argument("--samples", type=int, default=64, help="N: playouts of the gradient, a set of their own")
    f.add_argument("--prior", type=float, default=0.0, help="weight decay towards the start")
    f.add_argument("--scale", type=int, default=64, help="the pattern table's entry of gamma = 1")
    f.add_argument("--start-patterns", default=None, metavar="FILE", help="start from this pattern table (default: neutral)")
    f.add_argument("--start-tactics", default=None, metavar="FILE", help="start from this tactics table (default: neutral)")
    f.add_argument("--patterns-out", metavar="FILE", required=True, help="the pattern table, a .npy file")
    f.add_argument("--tactics-out", metavar="FILE", required=True, help="the tactics table, a .npy file")
    e.add_argument("--patterns", default=None, metavar="FILE")
    e.add_argument("--tactics", default=None, metavar="FILE")
    e.add_argument("--games", type=int, default=4096)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 0 <= args.seed < 2 ** 64:
        ap.error("--seed must be an unsigned 64-bit integer")
    if min(args.plies) < 0:
        ap.error("--plies must not be negative")
    if not 1 <= args.playouts <= MAX_COEF // 2:
        ap.error(f"--playouts must be 1..{MAX_COEF // 2}")
    if args.command == "fit":
        if args.games < 0 or (args.games == 0 and not args.records):
            ap.error("--games must be at least 1 (0 only with --records)")
        if args.games and not args.p:
            ap.error("-p POLICY is needed to play --games policy games")
        if args.iterations < 1:
            ap.error("--iterations must be at least 1")
        if not 0.0 < args.lr < float("inf"):
            ap.error("--lr must be positive")
        if args.samples < 1:
            ap.error("--samples must be at least 1")
        if not 0.0 <= args.prior < float("inf"):
            ap.error("--prior must not be negative")
        if not 1 <= args.scale <= 65535:
            ap.error("--scale must be 1..65535")
    else:
        if not args.p:
            ap.error("-p POLICY is needed to play the games")
        if args.games < 1:
            ap.error("--games must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    if args.command == "eval":
        pos, tgt, _, _ = labelled_positions(*RP.policy_games(args.p, args.games, args.seed, dev), plies=args.plies)
        r = value_error(pos, tgt, args.patterns, args.tactics, args.playouts, args.seed, device=dev)
        print(f"{r['positions']} positions at plies {args.plies}, N = {args.playouts}: mse {r['mse']:.4f}, sign agreement "
              f"{100 * r['agreement']:.1f} % (ties {100 * r['ties']:.1f} %)")
        return
    parts = []
    if args.games:
        parts.append(labelled_positions(*RP.policy_games(args.p, args.games, args.seed, dev), plies=args.plies))
    if args.records:
        parts.append(labelled_positions(*RP.record_games(args.records), plies=args.plies))
    pos, tgt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    start = strengths_of_tables(args.start_patterns, args.start_tactics, args.scale)
    f = fit(pos, tgt, args.iterations, args.lr, args.playouts, args.samples, start, args.prior, seed=args.seed, scale=args.scale,
            held_out=None, device=dev)
    for row in f.log[:-1]:
        print(f"iteration {row['iteration']:3d}: training mse {row['mse']:.4f}")
    f.patterns.save(args.patterns_out)
    f.tactics.save(args.tactics_out)
    print(f"{len(tgt)} positions -> {args.patterns_out}, {args.tactics_out}")
    print(TC.show(f.tactics))


if __name__ == "__main__":
    main()

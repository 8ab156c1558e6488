"""The joint fit of the playouts' two tables by minorization-maximization: the 3x3 pattern weights (patterns.py,
DESIGN 17) and the tactical weights (tactics.py) as ONE log-linear move model, fitted together.

    python -m bokego_amd.mmfit fit -p POLICY [--games 4096] [--seed S] [--records DIR ...] [--iterations 20] [--prior 1]
                                   [--scale 64] --patterns-out P.npy --tactics-out T.npy
    python -m bokego_amd.mmfit eval --patterns P.npy --tactics T.npy -p POLICY [--games N] [--seed S]

The playouts draw a playable point in proportion to w = max(1, (P * T) >> 8), P the pattern table's entry of the point's
3x3 index and T the tactics table's entry of its tactical code: a generalised Bradley-Terry model with two feature groups
and one feature of each group per candidate.  patterns.fit counts frequencies and tactics.fit takes one multiplicative
step on top of them; here both tables are the maximum of one penalised likelihood, found by Coulom's MM iteration
("Computing Elo Ratings of Move Patterns in the Game of Go", 2007): no learning rate, and every step raises the likelihood.

The iteration runs on integers.  A strength is g, uint32, gamma = g / 65536, 2^8 <= g <= 2^24.  One pass over the packed
plies (bkt_mm_sums; sums_host is the same in numpy, integer for integer) gives per ply the total strength E of the
candidates, the strength and the rank of the played move, and per feature den = the sum over plies and candidates that
carry it of floor(2^32 * team-mate's g / E).  One group is updated per pass -- its features are never team-mates of each
other, so the whole group moves at once --

    gamma <- (W + a) / (den / 2^32 + 2 a / (gamma + 1))

W the times the feature was played and a the prior: a virtual wins and a virtual losses against a feature of gamma = 1,
which also fixes the scale between the groups.  Patterns are pooled over the eight dihedral images of an index.  The update
itself is float64 on the host, from integers that are the same on both rules, so device and host fits agree bit for bit.

tables() rounds the strengths into the PatternTable and the TacticTable every consumer already loads; no fitted table
ships.
"""
import argparse
import collections

import numpy as np
import torch

from . import _trainlib as T
from . import lockstep as L
from . import patterns as PT
from . import replay as RP
from . import rollout as RO
from . import tactics as TC

G_ONE = 1 << 16                                    # gamma = 1
G_MIN, G_MAX = T.MM_G_MIN, T.MM_G_MAX
MAX_ROWS = T.MM_MAX_ROWS                           # rows of one bkt_mm_sums launch
MAX_FIT_ROWS = 1 << 22                             # plies of one fit: the sums stay below 2^63 (include/bokego_train.h)
PLAYABLE = np.uint32(1 << 31)
MOVE_NONE = T.MOVE_NONE

Group = collections.namedtuple("Group", "name entries shift bits pool")
Group.__doc__ = """A feature group of the model: `entries` strengths; a packed word holds the feature in `bits` bits from
bit `shift`; pool() is None or an int64 [entries] map of every feature to the one it shares its strength with."""
GROUPS = (Group("patterns", PT.ENTRIES, 0, 17, PT._canonical), Group("tactics", TC.ENTRIES, 17, 6, None))

Packed = collections.namedtuple("Packed", "codes moves played_p played_t")
Packed.__doc__ = """What pack returns: codes [R,81] and moves int32 [R] of every live ply -- numpy (codes uint32) with
rules="host", tensors on the device (codes int32, the same bits) with rules="device" -- and played_p int64
[patterns.ENTRIES], played_t int64 [tactics.ENTRIES] (numpy): how often each index and each code was played."""
Sums = collections.namedtuple("Sums", "den_p den_t total chosen rank")
Fit = collections.namedtuple("Fit", "gp gt log")

__all__ = ["GROUPS", "G_MAX", "G_MIN", "G_ONE", "MAX_FIT_ROWS", "MAX_ROWS", "Fit", "Packed", "Sums", "evaluate", "fit",
           "host", "pack", "pack_word", "penalised", "pooled", "step", "step_patterns", "step_tactics", "sums", "sums_host",
           "tables"]


# ---- the data -------------------------------------------------------------------------------------------------------------------
def pack_word(index, code, playable):
    """The word of a point (numpy): index | code << 17 | playable << 31, uint32."""
    word = np.asarray(index).astype(np.uint32) | np.asarray(code).astype(np.uint32) << np.uint32(17)
    return word | np.where(playable, PLAYABLE, np.uint32(0))


def pack(start_recs, moves, rules="device", device=None):
    """Replay the games once in lock-step -> Packed.  start_recs uint8 [G,192]; moves [G,L] as patterns.counts takes
    them.  A row per live ply (a move above MOVE_NONE; a pass has a row), per T.MAX_BATCH games ply by ply, the games of a
    ply in ascending order.  played_p and played_t count the moves that are playable board points, as patterns.counts and
    tactics.counts do.  rules="device": bkt_playout_step, bkt_pattern_codes, bkt_tactical_codes and torch bit operations;
    rules="host": the mirror on the host rules, the same integers."""
    L.check_rules(rules)
    start, moves = RP.check_games(start_recs, moves)
    parts = []
    if rules == "host":
        played = np.zeros(PT.ENTRIES, np.int64), np.zeros(TC.ENTRIES, np.int64)
        for _, _, live, recs, mv, ok in RP.replay_host(start, moves, T.MAX_BATCH):
            index, code = PT.codes_host(recs[live]), TC.codes_host(recs[live])
            parts.append((pack_word(index, code, ok), mv))
            at, good = RP.counted(mv, ok)
            for p, codes in zip(played, (index, code)):
                p += np.bincount(RP.at_move(codes, at)[good], minlength=len(p))
        if parts:
            return Packed(np.concatenate([c for c, _ in parts]), np.concatenate([m for _, m in parts]), *played)
        return Packed(np.zeros((0, 81), np.uint32), np.zeros(0, np.int32), *played)
    dev = RO._device(device, None, start_recs)
    played = (torch.zeros(PT.ENTRIES, dtype=torch.int64, device=dev), torch.zeros(TC.ENTRIES, dtype=torch.int64, device=dev))
    for _, _, pos, mv, live, playable in RP.replay_device(start, moves, dev):
        index, code = T.pattern_codes(pos), T.tactical_codes(pos)
        ok = playable != 0
        word = index | code << 17
        word = torch.where(ok, word | -(1 << 31), word)                  # bit 31 of the int32 that carries the uint32
        parts.append((word[live], mv[live]))
        at, good = RP.counted(mv, ok)
        good = live & good
        for p, codes in zip(played, (index, code)):
            p += torch.bincount(RP.at_move(codes, at)[good].to(torch.int64), minlength=len(p))
    played = (p.cpu().numpy() for p in played)
    if parts:
        return Packed(torch.cat([c for c, _ in parts]), torch.cat([m for _, m in parts]), *played)
    return Packed(torch.zeros((0, 81), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), *played)


def host(data):
    """A Packed with numpy codes (uint32) and moves, whichever rules made it."""
    if isinstance(data.codes, torch.Tensor):
        return Packed(data.codes.cpu().numpy().view(np.uint32), data.moves.cpu().numpy(), data.played_p, data.played_t)
    return data


# ---- one pass -------------------------------------------------------------------------------------------------------------------
def _strengths(g, entries, name):
    g = np.asarray(g)
    if g.shape != (entries,) or g.dtype.kind not in "iu":
        raise ValueError(f"{name} must be integers [{entries}], got {g.dtype} {g.shape}")
    if g.min() < G_MIN or g.max() > G_MAX:
        raise ValueError(f"{name}: a strength is {G_MIN}..{G_MAX} (gamma = g / 65536 in [2^-8, 2^8]), got {g.min()}..{g.max()}")
    return g.astype(np.uint64)


def _runs(index):
    """(order, first): a stable order that sorts index, and where each run of equal values starts in it."""
    order = np.argsort(index, kind="stable")
    sorted_index = index[order]
    return order, np.nonzero(np.r_[True, sorted_index[1:] != sorted_index[:-1]])[0]


def _add_at(out, index, value, runs=None):
    """out[index] += value for integer arrays, exactly (np.bincount would go through float64)."""
    if len(index):
        order, first = _runs(index) if runs is None else runs
        out[index[order[first]]] += np.add.reduceat(value[order], first)


def sums_host(codes, moves, gp, gt):
    """bkt_mm_sums in numpy, the definition (include/bokego_train.h says the same in words): codes uint32 [R,81], moves
    [R], gp [patterns.ENTRIES] and gt [tactics.ENTRIES] integers in G_MIN..G_MAX (else ValueError)
    -> Sums(den_p uint64 [patterns.ENTRIES], den_t uint64 [tactics.ENTRIES], total uint64 [R], chosen uint64 [R], rank
    int32 [R]).  Unsigned 64-bit integers throughout; nothing wraps inside the domain for R below MAX_FIT_ROWS."""
    codes, moves = np.asarray(codes), np.asarray(moves)
    if codes.ndim != 2 or codes.shape[1] != 81 or codes.dtype != np.uint32 or moves.shape != (len(codes),):
        raise ValueError("sums_host takes codes uint32 [R,81] and moves [R]")
    gp, gt = _strengths(gp, PT.ENTRIES, "gp"), _strengths(gt, TC.ENTRIES, "gt")
    n = len(codes)
    den_p, den_t = np.zeros(PT.ENTRIES, np.uint64), np.zeros(TC.ENTRIES, np.uint64)
    total, chosen, rank = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.full(n, -1, np.int32)
    for a in range(0, n, MAX_ROWS):
        word, mv = codes[a:a + MAX_ROWS], moves[a:a + MAX_ROWS].astype(np.int64)
        ok = (word >> np.uint32(31)) != 0
        index = (word & np.uint32(PT.ENTRIES - 1)).astype(np.int64)
        code = ((word >> np.uint32(17)) & np.uint32(TC.ENTRIES - 1)).astype(np.int64)
        s = np.where(ok, np.maximum((gp[index] * gt[code]) >> np.uint64(16), np.uint64(1)), np.uint64(0))
        E = s.sum(1, dtype=np.uint64)
        at, rows = np.clip(mv, 0, 80), np.arange(len(word))
        valid = (mv >= 0) & (mv <= 80) & ok[rows, at]
        s_m = np.where(valid, s[rows, at], np.uint64(0))
        total[a:a + MAX_ROWS], chosen[a:a + MAX_ROWS] = E, s_m
        rank[a:a + MAX_ROWS] = np.where(valid, RP.move_rank(s, s_m, mv, ok), -1)
        adds = ok & valid[:, None]
        Er = np.broadcast_to(np.maximum(E, np.uint64(1))[:, None], s.shape)[adds]   # E >= 1 on every row that adds
        _add_at(den_p, index[adds], (gt[code[adds]] << np.uint64(32)) // Er)
        _add_at(den_t, code[adds], (gp[index[adds]] << np.uint64(32)) // Er)
    return Sums(den_p, den_t, total, chosen, rank)


def sums(data, gp, gt, rules="device"):
    """One pass over a Packed -> Sums (numpy): rules="device": bkt_mm_sums (data from pack(rules="device"), or a host
    Packed, which is copied to the current device); rules="host": sums_host."""
    L.check_rules(rules)
    if rules == "host":
        d = host(data)
        return sums_host(d.codes, d.moves, gp, gt)
    codes, moves = data.codes, data.moves
    if not isinstance(codes, torch.Tensor):
        dev = torch.device("cuda", torch.cuda.current_device())
        codes, moves = torch.from_numpy(codes.view(np.int32)).to(dev), torch.from_numpy(np.asarray(moves, np.int32)).to(dev)
    out = T.mm_sums(codes, moves, np.asarray(gp), np.asarray(gt))
    den_p, den_t, total, chosen, rank = (t.cpu().numpy() for t in out)
    return Sums(den_p.view(np.uint64), den_t.view(np.uint64), total.view(np.uint64), chosen.view(np.uint64), rank)


# ---- the update -----------------------------------------------------------------------------------------------------------------
def _prior(prior):
    prior = float(prior)
    if not 0.0 < prior < float("inf"):
        raise ValueError("prior must be positive")
    return prior


def pooled(group, x):
    """x [entries] summed over the features that share a strength (exact integers), every feature holding its pool's sum."""
    x = np.asarray(x)
    if x.shape != (group.entries,) or x.dtype.kind not in "iu":
        raise ValueError(f"{group.name}: expected integers [{group.entries}]")
    if group.pool is None:
        return x
    canon = group.pool()
    if group.name not in _POOL_RUNS:
        _POOL_RUNS[group.name] = _runs(canon)
    out = np.zeros(group.entries, x.dtype)
    _add_at(out, canon, x, _POOL_RUNS[group.name])
    return out[canon]


_POOL_RUNS = {}


def step(group, g, played, den, prior=1.0):
    """One MM update of a whole group -> the new g, uint32 [entries]: with W = pooled played, D = pooled den / 2^32 and
    gamma = g / 65536,  gamma <- (W + a) / (D + 2 a / (gamma + 1)),  g = round(65536 gamma) clipped to G_MIN..G_MAX.
    float64 on the host.  A feature never seen (W = D = 0) moves to (gamma + 1) / 2: towards 1."""
    a = _prior(prior)
    gamma = _strengths(g, group.entries, "g").astype(np.float64) / G_ONE
    W = pooled(group, np.asarray(played, np.int64)).astype(np.float64)
    D = pooled(group, np.asarray(den, np.uint64)).astype(np.float64) / 2.0 ** 32
    new = (W + a) / (D + 2.0 * a / (gamma + 1.0))
    return np.clip(np.rint(new * G_ONE), G_MIN, G_MAX).astype(np.uint32)


def step_patterns(gp, played_p, den_p, prior=1.0):
    return step(GROUPS[0], gp, played_p, den_p, prior)


def step_tactics(gt, played_t, den_t, prior=1.0):
    return step(GROUPS[1], gt, played_t, den_t, prior)


def penalised(strengths, s, prior=1.0):
    """What a pass says about the tables it ran on -> dict: moves (the plies that count: the move a playable point),
    ll the sum of log(chosen / total) over them, penalised_ll = ll + the prior's term -- the sum over the distinct
    features of every group of a log(gamma) - 2 a log(gamma + 1) --, mean_ll = ll / moves, top1 and top5 the share of
    moves ranked first and among the first five.  float64 from the pass's integers."""
    a = _prior(prior)
    counts = s.rank >= 0
    n = int(counts.sum())
    ll = float(np.sum(np.log(s.chosen[counts].astype(np.float64)) - np.log(s.total[counts].astype(np.float64))))
    pen = 0.0
    for group, g in zip(GROUPS, strengths):
        gamma = np.asarray(g, np.float64) / G_ONE
        if group.pool is not None:
            gamma = gamma[group.pool() == np.arange(group.entries)]
        pen += float(np.sum(a * np.log(gamma) - 2.0 * a * np.log(gamma + 1.0)))
    return dict(moves=n, ll=ll, penalised_ll=ll + pen, mean_ll=ll / max(n, 1),
                top1=float((s.rank[counts] < 1).sum()) / max(n, 1), top5=float((s.rank[counts] < 5).sum()) / max(n, 1))


def fit(data, iterations=20, prior=1.0, rules="device"):
    """The joint fit -> Fit(gp uint32 [patterns.ENTRIES], gt uint32 [tactics.ENTRIES], log).  Every strength starts at
    G_ONE; an iteration is a pass that updates the patterns and a pass that updates the tactics.  log[h], h = 0 .. 2
    iterations, is penalised() of the tables after h half-iterations (the last one costs a pass of its own), with
    "iteration" = h / 2 and "updated" = the group the next half-iteration updates (None at the end).  The same data,
    iterations and prior give the same bits on both rules."""
    L.check_rules(rules)
    a, iterations = _prior(prior), int(iterations)
    if iterations < 0:
        raise ValueError("iterations must not be negative")
    rows = len(data.moves)
    if not 1 <= rows <= MAX_FIT_ROWS:
        raise ValueError(f"a fit takes 1..{MAX_FIT_ROWS} plies, got {rows}")
    g = [np.full(group.entries, G_ONE, np.uint32) for group in GROUPS]
    played = (data.played_p, data.played_t)
    log = []
    for h in range(2 * iterations + 1):
        s = sums(data, g[0], g[1], rules)
        k = h % len(GROUPS)
        last = h == 2 * iterations
        log.append(dict(penalised(g, s, a), iteration=h / 2, updated=None if last else GROUPS[k].name))
        if not last:
            g[k] = step(GROUPS[k], g[k], played[k], (s.den_p, s.den_t)[k], a)
    return Fit(g[0], g[1], log)


def tables(gp, gt, scale=64):
    """The strengths as the tables every consumer loads -> (PatternTable, TacticTable): pattern entries
    clip(round(scale gamma_p), 1, 65535) and tactics entries clip(round(256 gamma_t), 1, 65535), in exact integers.  The
    draw's w = (P T) >> 8 is then scale gamma_p gamma_t; scale = 64 takes the whole domain of gamma_p, up to 2^8, into
    uint16 without clipping at the top and leaves a pattern of gamma 1 six bits."""
    scale = int(scale)
    if not 1 <= scale <= 65535:
        raise ValueError("scale must be 1..65535")
    gp, gt = _strengths(gp, PT.ENTRIES, "gp").astype(np.int64), _strengths(gt, TC.ENTRIES, "gt").astype(np.int64)
    p = (2 * scale * gp + G_ONE) // (2 * G_ONE)
    t = (2 * TC.NEUTRAL * gt + G_ONE) // (2 * G_ONE)
    return PT.PatternTable(np.clip(p, 1, 65535).astype(np.uint16)), TC.TacticTable(np.clip(t, 1, 65535).astype(np.uint16))


# ---- the tables under the draw itself ---------------------------------------------------------------------------------------------
def evaluate(start_recs, moves, patterns=None, tactics=None, rules="device", device=None, plies=None):
    """How well a pair of TABLES predicts the moves of the games under the playouts' own draw -> dict(moves, mean_ll, top1,
    top5).  The games are replayed in lock-step and every position's weights come from rollout.move_weights (the existing
    kernel or its host mirror), so pairs from any fit compare directly, and so does a pair before and after tables()
    rounded it.  patterns, tactics: as rollout.move_weights takes them (None: none; both None is the uniform draw).  A ply
    counts when its move is a playable point; plies: None for all, or the ply numbers to count."""
    L.check_rules(rules)
    start, moves = RP.check_games(start_recs, moves)
    table, tac = RO._table(patterns), RO._tactics(tactics)
    want = None if plies is None else set(int(k) for k in plies)
    tally = dict(moves=0, ll=0.0, top1=0, top5=0)

    def count(w, mv):
        """The plies of one yield: w int64 [n,81] the weights of the draw before the moves mv [n]."""
        at, good = RP.counted(mv, w > 0)
        w_m = RP.at_move(w, at)
        rank = RP.move_rank(w, w_m, mv, w > 0)[good]
        tally["moves"] += int(good.sum())
        tally["ll"] += float(np.sum(np.log(w_m[good].astype(np.float64)) - np.log(w[good].sum(1).astype(np.float64))))
        tally["top1"] += int((rank < 1).sum())
        tally["top5"] += int((rank < 5).sum())

    if rules == "host":
        for k, _, live, recs, mv, _ in RP.replay_host(start, moves, T.MAX_BATCH, playable=False):
            if want is None or k in want:
                count(RO.move_weights_host(recs[live], table, tac).astype(np.int64), mv.astype(np.int64))
    else:
        for k, first, pos, _, _, _ in RP.replay_device(start, moves, RO._device(device, None, start_recs), playable=False):
            live = np.nonzero(moves[first:first + len(pos), k] > MOVE_NONE)[0]
            if len(live) and (want is None or k in want):
                count(RO._move_weights_device(pos, table, tac).cpu().numpy()[live].astype(np.int64),
                      moves[first + live, k].astype(np.int64))
    n = max(tally["moves"], 1)
    return dict(moves=tally["moves"], mean_ll=tally["ll"] / n, top1=tally["top1"] / n, top5=tally["top5"] / n)


# ---- the command line -----------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fit the pattern and the tactics table of the playouts together (MM), and evaluate a pair")
    sub = ap.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="fit both tables on policy playouts (and self-play records)")
    f.add_argument("-p", dest="p", metavar="POLICY", default=None, help="policy weights (.pt or .bkw); not needed with --games 0")
    f.add_argument("--games", type=int, default=4096, help="policy games from the empty board, played to the end")
    f.add_argument("--seed", type=int, default=0)
    f.add_argument("--records", nargs="+", default=None, metavar="DIR", help="selfplay --out directories to add")
    f.add_argument("--iterations", type=int, default=20, help="MM iterations: a patterns pass and a tactics pass each")
    f.add_argument("--prior", type=float, default=1.0, help="virtual wins and losses of every feature against gamma = 1")
    f.add_argument("--scale", type=int, default=64, help="the pattern table's entry of gamma = 1")
    f.add_argument("--device", type=int, default=0)
    f.add_argument("--patterns-out", metavar="FILE", required=True, help="the pattern table, a .npy file")
    f.add_argument("--tactics-out", metavar="FILE", required=True, help="the tactics table, a .npy file")
    e = sub.add_parser("eval", help="log-likelihood and top-1 / top-5 of a pair of tables on policy games")
    e.add_argument("--patterns", default=None, metavar="FILE")
    e.add_argument("--tactics", default=None, metavar="FILE")
    e.add_argument("-p", dest="p", metavar="POLICY", required=True, help="policy weights (.pt or .bkw)")
    e.add_argument("--games", type=int, default=4096)
    e.add_argument("--seed", type=int, default=1)
    e.add_argument("--device", type=int, default=0)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 0 <= args.seed < 2 ** 64:
        ap.error("--seed must be an unsigned 64-bit integer")
    if args.command == "fit":
        if args.games < 0 or (args.games == 0 and not args.records):
            ap.error("--games must be at least 1 (0 only with --records)")
        if args.games and not args.p:
            ap.error("-p POLICY is needed to play --games policy games")
        if args.iterations < 1:
            ap.error("--iterations must be at least 1")
        if not 0.0 < args.prior < float("inf"):
            ap.error("--prior must be positive")
        if not 1 <= args.scale <= 65535:
            ap.error("--scale must be 1..65535")
    elif args.games < 1:
        ap.error("--games must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    if args.command == "eval":
        r = evaluate(*RP.policy_games(args.p, args.games, args.seed, dev), args.patterns, args.tactics, device=dev)
        print(f"{r['moves']} moves: mean log-likelihood {r['mean_ll']:.4f}, top-1 {100 * r['top1']:.1f} %, top-5 {100 * r['top5']:.1f} %")
        return
    parts = []
    if args.games:
        parts.append(pack(*RP.policy_games(args.p, args.games, args.seed, dev), device=dev))
    if args.records:
        parts.append(pack(*RP.record_games(args.records), device=dev))
    data = Packed(torch.cat([p.codes for p in parts]), torch.cat([p.moves for p in parts]),
                  sum(p.played_p for p in parts), sum(p.played_t for p in parts))
    f = fit(data, args.iterations, args.prior)
    for row in f.log[::2]:
        print(f"iteration {row['iteration']:4.0f}: penalised log-likelihood {row['penalised_ll']:.2f}, mean {row['mean_ll']:.4f}, "
              f"top-1 {100 * row['top1']:.1f} %, top-5 {100 * row['top5']:.1f} %")
    table, tactics = tables(f.gp, f.gt, args.scale)
    table.save(args.patterns_out)
    tactics.save(args.tactics_out)
    print(f"{f.log[-1]['moves']} moves of {len(data.moves)} plies -> {args.patterns_out}, {args.tactics_out}")
    print(TC.show(tactics))


if __name__ == "__main__":
    main()

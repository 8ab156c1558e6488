"""Tactical playouts for the Monte-Carlo value: capture, escape and atari weights on top of the 3x3 patterns.

    python -m bokego_amd.tactics fit -p POLICY [--games 4096] [--seed S] [--patterns FILE] [--prior 16] -o tactics.npy
    python -m bokego_amd.tactics show tactics.npy

A 3x3 neighbourhood (patterns.py) cannot see how many liberties a chain has, so a pattern-weighted playout
leaves a stone in atari, declines a capture or plays a self-atari as often as the local shape suggests.  Here every point
of a record also gets a tactical code, and a second table of 64 weights multiplies the pattern weight of a playable point.

The code.  With F the 27 planes bk_features_batch_u8(record, fresh=0) gives -- the planes the policy net sees; a non-zero
entry of planes 6..26 holds the count, capped at 7 -- and q a point:
    cap = the value on planes 20..26 at q (stones captured by playing q), or 0;     C = min(cap, 3)
    la  = the value on planes 13..19 at q (liberties after playing q), 0: not legal; A = 0 for la <= 1, 1 for 2, 2 for >= 3
    E = 1 when some on-board 4-neighbour t has F[0][t] and F[6][t]: a stone of the side to move with one cached liberty
    G = 1 when some on-board 4-neighbour t has F[1][t] and F[7][t]: an opponent stone with two cached liberties
    code = C | A << 2 | E << 4 | G << 5                                               (A == 3 never occurs)
The liberty planes are the reference's cache and can be stale.  That is deliberate: the code is a function of the record's
bytes, so the host mirror (codes_host) equals the kernel (bkt_tactical_codes) bit for bit.

The draw.  A table is uint16 [ENTRIES]; NEUTRAL = 256 changes nothing.  For a playable point
    P = max(pattern entry, 1), or 256 without a pattern table;  T = tactics[code];  w = max(1, (P * T) >> 8)
(w < 2^24, so a row's sum S <= 81 * 2^24 < 2^31) and the rest is patterns.py's draw on the same Philox word:
t = ((x0 >> 8) * S) >> 24, the first playable point whose inclusive prefix sum of w exceeds t, a pass when there is none.
A neutral table plays the pattern games, and without a pattern table the uniform games, byte for byte.

The fit is one multiplicative-update step on top of the pattern table: weights = 256 * played / mass, where played[code]
counts the moves played and mass[code] is the number of plays the pattern-only draw expects of that code on the same
plies (each playable point adds P / the sum of P over the playable points).  Counting plain frequencies instead would count
the shape information twice.  That step is the first of a minorization-maximization iteration and stops there, with the
pattern table fixed; mmfit.py carries the iteration on over both tables and writes this module's table
format.  No fitted table ships.
"""
import argparse

import numpy as np
import torch

from . import _trainlib as T
from . import lockstep as L
from . import patterns as PT
from . import replay as RP
from . import rollout as RO

ENTRIES = T.TACTIC_ENTRIES
NEUTRAL = 256

__all__ = ["ENTRIES", "NEUTRAL", "TacticTable", "as_tactics", "codes_host", "combine", "counts", "describe", "fit",
           "select_tactical", "weights"]


# ---- the code -------------------------------------------------------------------------------------------------------------------
def _near(flag):
    """bool [n,81] -> bool [n,81]: some on-board 4-neighbour of the point has the flag."""
    pad = np.zeros((len(flag), 11, 11), bool)
    pad[:, 1:10, 1:10] = flag.reshape(-1, 9, 9)
    return (pad[:, :9, 1:10] | pad[:, 2:, 1:10] | pad[:, 1:10, :9] | pad[:, 1:10, 2:]).reshape(-1, 81)


def codes_host(recs):
    """The tactical code of every point of every record, occupied or not: recs uint8 [n,192] (numpy; not modified) ->
    int32 [n,81]; the mirror of bkt_tactical_codes."""
    recs = np.array(recs, np.uint8, order="C")                        # a copy: the encoder refreshes the liberty cache in place
    n = len(recs)
    F = np.empty((n, 27, 81), np.uint8)
    if n:
        L.features_batch(recs, F.ctypes.data)
    cap = F[:, 20:27].max(1).astype(np.int32)
    la = F[:, 13:20].max(1).astype(np.int32)
    C = np.minimum(cap, 3)
    A = np.where(la <= 1, 0, np.where(la == 2, 1, 2))
    E = _near((F[:, 0] != 0) & (F[:, 6] != 0))
    G = _near((F[:, 1] != 0) & (F[:, 7] != 0))
    return (C | A << 2 | E.astype(np.int32) << 4 | G.astype(np.int32) << 5).astype(np.int32)


def describe(code):
    """One line of words for a code."""
    c, a, e, g = code & 3, (code >> 2) & 3, (code >> 4) & 1, (code >> 5) & 1
    parts = [("captures 3+" if c == 3 else f"captures {c}") if c else "no capture",
             {0: "at most 1 liberty after (or not legal)", 1: "2 liberties after", 2: "3+ liberties after", 3: "(unused)"}[a]]
    if e:
        parts.append("next to an own chain in atari")
    if g:
        parts.append("next to an opponent chain with 2 liberties")
    return ", ".join(parts)


# ---- the draw -------------------------------------------------------------------------------------------------------------------
def _pattern_weight(pattern_entries, shape=None):
    """P of the draw, uint64: max(entry, 1), or 256 everywhere (of `shape`) without a pattern table."""
    if pattern_entries is None:
        return np.uint64(NEUTRAL) if shape is None else np.full(shape, NEUTRAL, np.uint64)
    return np.maximum(np.asarray(pattern_entries).astype(np.uint64), np.uint64(1))


def combine(pattern_entries, tactic_entries):
    """w = max(1, (P * T) >> 8), uint64, elementwise: pattern_entries the pattern table's entries of the points (None: no
    pattern table, P = 256), tactic_entries the tactics table's entries of their codes.  w <= 65535^2 >> 8 < 2^24."""
    t = np.asarray(tactic_entries).astype(np.uint64)
    return np.maximum((_pattern_weight(pattern_entries) * t) >> np.uint64(8), np.uint64(1))


def select_tactical(x0, pattern_entries, tactic_entries, playable):
    """The move of each row, int64 [R]: x0 uint32 [R], pattern_entries [R,81] or None, tactic_entries [R,81], playable
    bool [R,81].  patterns.select_weighted (its threshold and prefix-sum rule) on the combined weights; go.PASS where a row
    has no playable point."""
    return PT.select_weighted(x0, combine(pattern_entries, tactic_entries), playable)


# ---- the table ------------------------------------------------------------------------------------------------------------------
class TacticTable(PT.WeightTable):
    """The weights indexed by the tactical code, 256 = neutral (bkt_tactical_playouts)."""
    ENTRIES, NOUN = ENTRIES, "tactics"

    @classmethod
    def neutral(cls):
        return cls(np.full(ENTRIES, NEUTRAL, np.uint16))


as_tactics = TacticTable.coerce         # None, a TacticTable, a uint16 [ENTRIES] array or the path of a saved table


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def counts(start_recs, moves, patterns=None, rules="device", device=None):
    """Replay the games in lock-step -> (mass float64 [ENTRIES], played int64 [ENTRIES]) (numpy).  start_recs uint8
    [G,192]; moves [G,L] as patterns.counts takes them.  Per ply of a game, played[code] goes up by one for the move, if
    it is a playable board point, and mass[code] by P / (the sum of P over the playable points) for every playable point,
    P = max(pattern entry, 1) with patterns (what patterns.as_table takes), 1 / n without: the number of plays the
    pattern-only draw expects of each code.  rules="device": bkt_playout_step, bkt_tactical_codes, bkt_pattern_codes and
    torch reductions; rules="host": the mirror.  played is the same integers on both; mass sums the same float64 terms
    in another order."""
    L.check_rules(rules)
    table = PT.as_table(patterns)
    start, moves = RP.check_games(start_recs, moves)
    if rules == "host":
        mass, played = np.zeros(ENTRIES, np.float64), np.zeros(ENTRIES, np.int64)
        for _, _, live, recs, mv, ok in RP.replay_host(start, moves):
            codes = codes_host(recs[live])
            P = ok.astype(np.float64)
            if table is not None:
                P = P * np.maximum(table.entries(PT.codes_host(recs[live])), 1).astype(np.float64)
            share = P / np.maximum(P.sum(1, keepdims=True), 1.0)
            mass += np.bincount(codes[ok], weights=share[ok], minlength=ENTRIES)
            at, good = RP.counted(mv, ok)
            played += np.bincount(RP.at_move(codes, at)[good], minlength=ENTRIES)
        return mass, played
    dev = RO._device(device, None, start_recs)
    mass = torch.zeros(ENTRIES, dtype=torch.float64, device=dev)
    played = torch.zeros(ENTRIES, dtype=torch.int64, device=dev)
    w = None if table is None else (table.device(dev).to(torch.int64) & 0xFFFF).clamp_(min=1).to(torch.float64)
    for _, _, pos, mv, live, playable in RP.replay_device(start, moves, dev):
        codes = T.tactical_codes(pos).to(torch.int64)
        ok = (playable != 0) & live[:, None]
        P = ok.to(torch.float64) if w is None else w[T.pattern_codes(pos).to(torch.int64)] * ok
        share = P / P.sum(1, keepdim=True).clamp_(min=1.0)                   # a row without a playable point adds nothing
        mass += torch.bincount(codes[ok], weights=share[ok], minlength=ENTRIES)
        at, good = RP.counted(mv, ok)
        played += torch.bincount(RP.at_move(codes, at)[good], minlength=ENTRIES)
    return mass.cpu().numpy(), played.cpu().numpy()


def weights(mass, played, prior=16.0):
    """The table of a fit: floor(256 * (played + prior) / (mass + prior) + 1/2), clipped to 1..65535.  prior > 0 is a
    count of plays that the pattern-only draw is taken to have predicted exactly: a code never available stays neutral."""
    prior = float(prior)
    if not prior > 0:
        raise ValueError("prior must be positive")
    mass, played = np.asarray(mass, np.float64), np.asarray(played, np.float64)
    w = np.floor(NEUTRAL * (played + prior) / (mass + prior) + 0.5)
    return np.clip(w, 1, 65535).astype(np.uint16)


def fit(start_recs, moves, patterns=None, rules="device", device=None, prior=16.0):
    """counts -> weights -> a TacticTable, on top of the pattern table `patterns` (or of none)."""
    return TacticTable(weights(*counts(start_recs, moves, patterns, rules, device), prior=prior))


# ---- the command line -----------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fit and inspect the tactical weights of the Monte-Carlo playouts")
    sub = ap.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="fit a table on policy playouts, on top of a pattern table")
    f.add_argument("-p", dest="p", metavar="POLICY", required=True, help="policy weights (.pt or .bkw)")
    f.add_argument("--games", type=int, default=4096, help="policy games from the empty board, played to the end")
    f.add_argument("--seed", type=int, default=0)
    f.add_argument("--patterns", default=None, metavar="FILE",
                   help="the pattern table the playouts will use (python -m bokego_amd.patterns fit); default: none")
    f.add_argument("--prior", type=float, default=16.0, help="prior count of a code (weights)")
    f.add_argument("--device", type=int, default=0)
    f.add_argument("-o", dest="o", metavar="FILE", required=True, help="the table, a .npy file")
    s = sub.add_parser("show", help="print the entries of a table that are not neutral")
    s.add_argument("table")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.command == "fit":
        if args.games < 1:
            ap.error("--games must be at least 1")
        if not 0 <= args.seed < 2 ** 64:
            ap.error("--seed must be an unsigned 64-bit integer")
        if not args.prior > 0:
            ap.error("--prior must be positive")
    return args


def show(table):
    """The text `show` prints: every code whose entry is not neutral (A == 3 never occurs), heaviest first."""
    order = sorted((c for c in range(ENTRIES) if (c >> 2) & 3 != 3 and table.array[c] != NEUTRAL),
                   key=lambda c: (-int(table.array[c]), c))
    lines = [f"code {c:2d}  x{table.array[c] / NEUTRAL:7.3f}  {describe(c)}" for c in order]
    return "\n".join(lines) if lines else "every entry is neutral"


def main(argv=None):
    args = parse_args(argv)
    if args.command == "show":
        print(show(TacticTable.load(args.table)))
        return
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    mass, played = counts(*RP.policy_games(args.p, args.games, args.seed, dev), args.patterns, device=dev)
    table = TacticTable(weights(mass, played, prior=args.prior))
    table.save(args.o)
    print(f"{int(played.sum())} moves, {int((played > 0).sum())} codes played -> {args.o}")
    print(show(table))


if __name__ == "__main__":
    main()

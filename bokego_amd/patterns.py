"""Pattern-weighted playouts for the Monte-Carlo value: the 3x3 pattern index, the weighted integer draw, the
table of weights and its fit from games.

    python -m bokego_amd.patterns fit -p POLICY [--games 4096] [--seed S] [--records DIR ...] -o table.npy
    python -m bokego_amd.patterns show table.npy [-n 8]

A uniformly random playout (rollout.random_playouts) is blind to shape.  Here a move is drawn in proportion to a
weight looked up from its 3x3 neighbourhood, as MoGo's patterns and AlphaGo's fast rollout policy do, and the weights are
fitted by counting how often each pattern was played when it was available.

The index of a point s = 9r + c of a bk_pos record, relative to the record's side to move: the eight neighbours in the
order NEIGHBOURS give a 2-bit state each (0 empty, 1 a stone of the side to move, 2 an opponent stone, 3 off the board),
code = sum of state_i << 2i; near = 1 when the record's last move is a board point at most one step away in both
directions (a pass or no move: 0); index = near << 16 | code.  A table is uint16[ENTRIES], 256 KB; the weight of a point is
max(entry, 1), so every playable point can be drawn and no table is invalid.

The draw at a ply with the playable set P and the Philox word x0 of rollout.random_playouts: S = the sum of the weights
over P (< 2^23), t = ((x0 >> 8) * S) >> 24 in 64-bit integers, and the move is the first point of P, in ascending order,
whose inclusive prefix sum of weights exceeds t; a pass when P is empty.  No float, no fallback rule: the host mirror
(codes_host, select_weighted) equals the kernels (bkt_pattern_codes, bkt_pattern_playouts) bit for bit.  A table of one
constant c selects rank floor(floor(u c n / 2^24) / c) = floor(u n / 2^24): random_playouts' own game.

rollout.random_playouts, playout_value and PlayoutEvaluator take a table as patterns=; this module holds what they need
and the fit.  No fitted table ships: `fit` makes one in about a second.  `fit` counts frequencies, played / seen, and
knows nothing of the tactics table that multiplies its weights; mmfit.py fits both tables together as one
model and writes this module's table format.
"""
import argparse

import numpy as np
import torch

from . import _trainlib as T
from . import go
from . import lockstep as L
from . import replay as RP
from . import rollout as RO
from .replay import record_games  # noqa: F401  (its name here, as the command lines of the fits know it)

ENTRIES = T.PATTERN_ENTRIES                                            # 2 * 4^8
NEAR = 1 << 16
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))      # slot i: (dr, dc)
# The dihedral group of the square as integer matrices (a, b, c, d): (dr, dc) -> (a dr + b dc, c dr + d dc).
SYMMETRIES = ((1, 0, 0, 1), (0, -1, 1, 0), (-1, 0, 0, -1), (0, 1, -1, 0), (1, 0, 0, -1), (-1, 0, 0, 1), (0, 1, 1, 0),
              (0, -1, -1, 0))

__all__ = ["ENTRIES", "NEIGHBOURS", "SYMMETRIES", "PatternTable", "as_table", "codes_host", "counts", "picture",
           "select_weighted", "slot_permutation", "symmetrise", "transform_code", "transform_point", "weighted_pick",
           "weights"]


# ---- the index ------------------------------------------------------------------------------------------------------------------
def codes_host(recs):
    """The pattern index of every point of every record, occupied or not: recs uint8 [n,192] (numpy) -> int32 [n,81]; the
    mirror of bkt_pattern_codes."""
    recs = np.asarray(recs, np.uint8)
    n = len(recs)
    board = recs[:, :81].reshape(n, 9, 9)
    mover = np.where(L.black_to_move(recs), 1, 2).astype(np.uint8)[:, None, None]
    state = np.full((n, 11, 11), 3, np.int32)
    state[:, 1:10, 1:10] = np.where(board == 0, 0, np.where(board == mover, 1, 2))
    code = np.zeros((n, 9, 9), np.int32)
    for i, (dr, dc) in enumerate(NEIGHBOURS):
        code |= state[:, 1 + dr:10 + dr, 1 + dc:10 + dc] << (2 * i)
    lm = L.record_last_move(recs).astype(np.int32)
    on_board = (lm >= 0) & (lm < 81)
    rl, cl = (np.where(on_board, lm, 0) // 9)[:, None, None], (np.where(on_board, lm, 0) % 9)[:, None, None]
    r, c = np.arange(9)[None, :, None], np.arange(9)[None, None, :]
    near = on_board[:, None, None] & (np.abs(r - rl) <= 1) & (np.abs(c - cl) <= 1)
    return (code | np.where(near, NEAR, 0)).reshape(n, 81).astype(np.int32)


def slot_permutation(g):
    """perm [8]: under symmetry g (an index into SYMMETRIES) the neighbour in slot i lands in slot perm[i]."""
    a, b, c, d = SYMMETRIES[g]
    return [NEIGHBOURS.index((a * dr + b * dc, c * dr + d * dc)) for dr, dc in NEIGHBOURS]


def transform_code(code, g):
    """The index of the same point after the board has been transformed by symmetry g: the slots permuted, near kept."""
    code = np.asarray(code, np.int64)
    out = code & NEAR
    for i, j in enumerate(slot_permutation(g)):
        out = out | (((code >> (2 * i)) & 3) << (2 * j))
    return out


def transform_point(s, g):
    """The point that s = 9r + c lands on under symmetry g (about the centre of the board); a pass or no move stays."""
    s = np.asarray(s, np.int64)
    a, b, c, d = SYMMETRIES[g]
    r, col = s // 9 - 4, s % 9 - 4
    return np.where((s >= 0) & (s < 81), 9 * (a * r + b * col + 4) + (c * r + d * col + 4), s)


# ---- the draw -------------------------------------------------------------------------------------------------------------------
def _threshold(x0, S):
    return ((np.asarray(x0, np.uint64) >> np.uint64(8)) * np.asarray(S, np.uint64)) >> np.uint64(24)


def weighted_pick(x0, weights_of_P):
    """The rank, among the playable points in ascending order, that the Philox word x0 selects: weights_of_P [n] are their
    table entries (an entry of 0 counts as 1); t = ((x0 >> 8) * S) >> 24 with S their sum, and the rank is the first whose
    inclusive prefix sum exceeds t.  n must be at least 1.  S <= 81 * 65535 < 2^23, so the product has at most 47 bits."""
    w = np.maximum(np.asarray(weights_of_P, np.uint64), np.uint64(1))
    if w.ndim != 1 or len(w) < 1:
        raise ValueError("weighted_pick takes the weights of at least one playable point")
    c = np.cumsum(w, dtype=np.uint64)
    return int(np.argmax(c > _threshold(x0, c[-1])))


def select_weighted(x0, entries, playable):
    """weighted_pick for rows: x0 uint32 [R], entries [R,81] (the table entry of every point), playable bool [R,81]
    -> the move of each row, int64 [R]: a point, or go.PASS where a row has no playable point."""
    w = np.where(playable, np.maximum(np.asarray(entries, np.uint64), np.uint64(1)), np.uint64(0)).astype(np.uint64)
    c = np.cumsum(w, 1, dtype=np.uint64)
    pick = np.argmax(c > _threshold(x0, c[:, -1])[:, None], 1)
    return np.where(c[:, -1] > 0, pick, go.PASS)


# ---- the table ------------------------------------------------------------------------------------------------------------------
class WeightTable:
    """uint16 [ENTRIES] weights of the playouts' draw; a subclass names its ENTRIES and its NOUN.  device(dev) is a cached
    copy for the playout kernels."""
    ENTRIES = NOUN = None

    def __init__(self, array):
        array = np.asarray(array)
        if array.shape != (self.ENTRIES,) or array.dtype != np.uint16:
            raise ValueError(f"a {self.NOUN} table is uint16 [{self.ENTRIES}], got {array.dtype} {array.shape}")
        self.array = np.ascontiguousarray(array)
        self._device = {}

    @classmethod
    def load(cls, path):
        return cls(np.load(path, allow_pickle=False))

    @classmethod
    def coerce(cls, table):
        """None, a table of this class, a uint16 [ENTRIES] array or the path of a saved table -> None or a table."""
        if table is None or isinstance(table, cls):
            return table
        return cls(table) if isinstance(table, np.ndarray) else cls.load(table)

    def save(self, path):
        with open(path, "wb") as f:                                   # an open file: np.save appends no suffix
            np.save(f, self.array, allow_pickle=False)

    def entries(self, codes):
        """The table entry of every index of codes (numpy)."""
        return self.array[codes]

    def device(self, dev):
        """int16 [ENTRIES] on dev holding the bits of the weights (what _trainlib's playouts take)."""
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            self._device[dev] = torch.from_numpy(self.array.view(np.int16).copy()).to(dev)
        return self._device[dev]


class PatternTable(WeightTable):
    """The weights indexed by the pattern index (bkt_pattern_playouts)."""
    ENTRIES, NOUN = ENTRIES, "pattern"

    @classmethod
    def constant(cls, c):
        if not 0 <= int(c) <= 65535:
            raise ValueError("a weight is 0..65535")
        return cls(np.full(ENTRIES, int(c), np.uint16))


as_table = PatternTable.coerce          # None, a PatternTable, a uint16 [ENTRIES] array or the path of a saved table


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def counts(start_recs, moves, rules="device", device=None):
    """Replay the games in lock-step and count patterns -> (seen, played), both int64 [ENTRIES] (numpy).
    start_recs uint8 [G,192]; moves [G,L]: the move of each ply, a point, go.PASS, or MOVE_NONE once a game is over (the
    history finish_games returns).  Per ply of a game, seen[index] goes up by one for each playable point (legal, and not
    the mover's own eye), and played[index] for the move -- if it is a playable board point: self-play records may fill an
    eye, and such a ply adds to seen only.  rules="device": bkt_playout_step, bkt_pattern_codes and torch.bincount;
    rules="host": the mirror on the host rules, the same integers."""
    L.check_rules(rules)
    start, moves = RP.check_games(start_recs, moves)
    if rules == "host":
        seen, played = np.zeros(ENTRIES, np.int64), np.zeros(ENTRIES, np.int64)
        for _, _, live, recs, mv, ok in RP.replay_host(start, moves):
            codes = codes_host(recs[live])
            seen += np.bincount(codes[ok], minlength=ENTRIES)
            at, good = RP.counted(mv, ok)
            played += np.bincount(RP.at_move(codes, at)[good], minlength=ENTRIES)
        return seen, played
    dev = RO._device(device, None, start_recs)
    seen = torch.zeros(ENTRIES, dtype=torch.int64, device=dev)
    played = torch.zeros(ENTRIES, dtype=torch.int64, device=dev)
    for _, _, pos, mv, live, playable in RP.replay_device(start, moves, dev):
        codes = T.pattern_codes(pos).to(torch.int64)
        ok = (playable != 0) & live[:, None]
        seen += torch.bincount(codes[ok], minlength=ENTRIES)
        at, good = RP.counted(mv, ok)                # (launched while the bincount runs; before it, the ply waits 20 us longer)
        played += torch.bincount(RP.at_move(codes, at)[good], minlength=ENTRIES)
    return seen.cpu().numpy(), played.cpu().numpy()


_CANONICAL = None


def _canonical():
    """int64 [ENTRIES]: the smallest index among the 8 dihedral images of each index (one name per orbit)."""
    global _CANONICAL
    if _CANONICAL is None:
        idx = np.arange(ENTRIES, dtype=np.int64)
        _CANONICAL = np.min([transform_code(idx, g) for g in range(8)], 0)
    return _CANONICAL


def symmetrise(seen, played):
    """Each index gets the sum of the counts over its distinct dihedral images -> (seen, played), int64 [ENTRIES].  The
    dihedral action is slot_permutation on the 8 neighbour slots; near is invariant."""
    canon = _canonical()
    out = []
    for a in (seen, played):
        a = np.asarray(a, np.int64)
        if a.shape != (ENTRIES,):
            raise ValueError(f"counts are int64 [{ENTRIES}]")
        orbit = np.zeros(ENTRIES, np.int64)
        np.add.at(orbit, canon, a)
        out.append(orbit[canon])
    return tuple(out)


def weights(seen, played, scale=1024, prior_played=1, prior_seen=32):
    """The table of a fit: round(scale * (played + prior_played) / (seen + prior_seen)) in exact integers --
    (2 scale (played + prior_played) + (seen + prior_seen)) // (2 (seen + prior_seen)) -- clipped to 1..65535.  A pattern
    never seen gets the prior rate."""
    seen, played = np.asarray(seen, np.int64), np.asarray(played, np.int64)
    den = seen + int(prior_seen)
    w = (2 * int(scale) * (played + int(prior_played)) + den) // (2 * den)
    return np.clip(w, 1, 65535).astype(np.uint16)


def fit(start_recs, moves, rules="device", device=None, **kw):
    """counts -> symmetrise -> weights -> a PatternTable."""
    return PatternTable(weights(*symmetrise(*counts(start_recs, moves, rules, device)), **kw))


# ---- the command line -----------------------------------------------------------------------------------------------------------
def picture(index):
    """Three lines: the neighbourhood of a pattern index, X the side to move, O the opponent, # off the board, and the
    point itself * when the last move is near, + otherwise."""
    cell = {(dr, dc): ".XO#"[(index >> (2 * i)) & 3] for i, (dr, dc) in enumerate(NEIGHBOURS)}
    cell[(0, 0)] = "*" if index & NEAR else "+"
    return "\n".join(" ".join(cell[(dr, dc)] for dc in (-1, 0, 1)) for dr in (-1, 0, 1))


def build_parser():
    ap = argparse.ArgumentParser(description="Fit and inspect the 3x3 pattern weights of the Monte-Carlo playouts")
    sub = ap.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="fit a table on policy playouts (and self-play records)")
    f.add_argument("-p", dest="p", metavar="POLICY", required=True, help="policy weights (.pt or .bkw)")
    f.add_argument("--games", type=int, default=4096, help="policy games from the empty board, played to the end")
    f.add_argument("--seed", type=int, default=0)
    f.add_argument("--records", nargs="+", default=None, metavar="DIR", help="selfplay --out directories to add")
    f.add_argument("--scale", type=int, default=1024, help="the weight of a pattern that is always played")
    f.add_argument("--device", type=int, default=0)
    f.add_argument("-o", dest="o", metavar="FILE", required=True, help="the table, a .npy file")
    s = sub.add_parser("show", help="print the heaviest and the lightest patterns of a table")
    s.add_argument("table")
    s.add_argument("-n", dest="n", type=int, default=8, help="patterns per end")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.command == "fit":
        if args.games < 0 or (args.games == 0 and not args.records):
            ap.error("--games must be at least 1 (0 only with --records)")
        if not 0 <= args.seed < 2 ** 64:
            ap.error("--seed must be an unsigned 64-bit integer")
        if not 1 <= args.scale <= 65535:
            ap.error("--scale must be 1..65535")
    elif args.n < 1:
        ap.error("-n must be at least 1")
    return args


def show(table, n=8):
    """The text `show` prints: the n heaviest and the n lightest distinct patterns (one per dihedral orbit)."""
    canon = _canonical()
    idx = np.nonzero(canon == np.arange(ENTRIES))[0]
    order = idx[np.argsort(table.array[idx].astype(np.int64), kind="stable")]
    lines = []
    for title, part in (("heaviest", order[::-1][:n]), ("lightest", order[:n])):
        lines.append(f"{title}:")
        for i in part.tolist():
            lines.append(f"index {i}  weight {max(int(table.array[i]), 1)}")
            lines.append(picture(i))
    return "\n".join(lines)


def main(argv=None):
    args = parse_args(argv)
    if args.command == "show":
        print(show(PatternTable.load(args.table), args.n))
        return
    torch.cuda.set_device(args.device)
    dev = torch.device("cuda", args.device)
    seen, played = np.zeros(ENTRIES, np.int64), np.zeros(ENTRIES, np.int64)
    if args.games:
        seen, played = counts(*RP.policy_games(args.p, args.games, args.seed, dev), device=dev)
    if args.records:
        more = counts(*record_games(args.records), device=dev)
        seen, played = seen + more[0], played + more[1]
    table = PatternTable(weights(*symmetrise(seen, played), scale=args.scale))
    table.save(args.o)
    print(f"{int(played.sum())} moves, {int(seen.sum())} playable points, {int((seen > 0).sum())} patterns seen -> {args.o}")


if __name__ == "__main__":
    main()

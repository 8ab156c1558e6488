"""The move-context table of the NAST playouts (the N-gram average sampling technique, Powley, Whitehouse & Cowling 2013; the
N-gram selection of Tak, Winands & Bjornsson 2012), its host mirror and the two rules in numpy.
include/bokego_train.h has the definition the kernels, this module and the docs share:

    counts int64 [2,82,81,2]  counts[c, p, m] = (played, won) of colour c (0 black, 1 white) on point m played directly
                              after move p, by either side; p == 81: after anything -- movevalues.MoveValueTable's counts
    values uint16 [2,82,81]   the factor of the draw's weight in units of 1/256: 256 neutral, every entry >= 1
    lut, k, limit             exactly the move-value table's (movevalues.lut_of, check_k_limit)
    min_plays                 1..MAX_MIN_PLAYS: the plays a context entry needs before it counts
    previous move             the move played immediately before, a pass included; the record's last move at ply 0;
                              anything outside 0..80 (a pass, none, junk) is plane 81
    use     (move_context_weights)      w = min(2^24 - 1, max(1, (w_in * values[c, p, q]) >> 8))
    update  (move_context_update_host)  every play counts for (c, 81, m), and for (c, p, m) when p < 81; then, per entry:
                                        halved until played < limit (limit > 0); i1 = rate_index of plane 81 and
                                        values[c, 81, m] = lut[i1]; for p < 81, values[c, p, m] = lut[(i1 + i2) >> 1] when
                                        the entry's played >= min_plays, i2 its own rate_index, else values[c, 81, m]

Everything is an integer: the device computes the same bits.  rollout.py's playouts take a MoveContextTable as move_values=
and update it in place (bkt_move_context_playouts, bkt_move_context_update); the host/device liveness rule is
MoveValueTable's.
"""
import numpy as np

from . import lockstep as L
from .movevalues import (DEFAULT_K, DEFAULT_LIMIT, DEFAULT_TAU, MOVE_NONE, NEUTRAL, WEIGHT_CAP, MoveValueTable, check_k_limit,
                         lut_of, rate_index)

PLANES = 82                # 81 previous moves and plane 81, the move-value table
MAX_MIN_PLAYS = 1 << 30    # BKT_MOVE_CONTEXT_MAX_MIN_PLAYS
DEFAULT_MIN_PLAYS = 8      # plausible and untuned (Tak et al. use 7)

__all__ = ["PLANES", "MAX_MIN_PLAYS", "DEFAULT_MIN_PLAYS", "MoveContextTable", "check_min_plays", "context_of",
           "move_context_weights", "move_context_update_host"]


def check_min_plays(min_plays):
    """min_plays as an int in the domain of bkt_move_context_update: 1..MAX_MIN_PLAYS (ValueError)."""
    if isinstance(min_plays, bool) or not isinstance(min_plays, (int, np.integer)):
        raise TypeError(f"min_plays, the plays a context entry needs before it counts, must be an int, got {type(min_plays).__name__}")
    if not 1 <= min_plays <= MAX_MIN_PLAYS:
        raise ValueError(f"min_plays, the plays a context entry needs before it counts, must be 1..{MAX_MIN_PLAYS}, got {min_plays}")
    return int(min_plays)


def context_of(prev):
    """The plane of a previous move, int64 elementwise: the move itself when it is a board point 0..80, else 81 (a pass,
    none, junk) -- compared before it indexes."""
    prev = np.asarray(prev).astype(np.int64)
    return np.where((prev >= 0) & (prev <= 80), prev, 81)


class MoveContextTable(MoveValueTable):
    """counts int64 [2,82,81,2], values uint16 [2,82,81], lut uint16 [65], k, limit and min_plays (module docstring).
    `.counts`, `.values`, device(dev), clear(), occupancy(), deepcopy, pickle and the host/device liveness rule are
    MoveValueTable's; move_values() is plane 81 as a MoveValueTable of its own (a copy)."""

    def __init__(self, counts, values, lut, k=DEFAULT_K, limit=DEFAULT_LIMIT, min_plays=DEFAULT_MIN_PLAYS):
        counts, values, lut = np.asarray(counts), np.asarray(values), np.asarray(lut)
        if counts.shape != (2, PLANES, 81, 2) or counts.dtype != np.int64:
            raise ValueError(f"the counts of a move-context table are int64 [2, 82, 81, 2], got {counts.dtype} {counts.shape}")
        if values.shape != (2, PLANES, 81) or values.dtype != np.uint16 or (values < 1).any():
            raise ValueError(f"the values of a move-context table are uint16 [2, 82, 81], every entry >= 1, got {values.dtype} {values.shape}")
        if lut.shape != (65,) or lut.dtype != np.uint16 or (lut < 1).any():
            raise ValueError(f"the lut of a move-context table is uint16 [65], every entry >= 1, got {lut.dtype} {lut.shape}")
        if (counts < 0).any() or (counts[..., 1] > counts[..., 0]).any():
            raise ValueError("the counts of a move-context table are 0 <= won <= played")
        self.k, self.limit = check_k_limit(k, limit)
        self.min_plays = check_min_plays(min_plays)
        self._counts = np.array(counts, np.int64, order="C")
        self._values = np.array(values, np.uint16, order="C")
        self.lut = np.array(lut, np.uint16, order="C")
        self.lut.setflags(write=False)
        self._device = {}
        self._live = None

    @classmethod
    def empty(cls, tau=DEFAULT_TAU, k=DEFAULT_K, limit=DEFAULT_LIMIT, min_plays=DEFAULT_MIN_PLAYS):
        """No play counted, every value lut_of(tau)[32] == 256."""
        return cls(np.zeros((2, PLANES, 81, 2), np.int64), np.full((2, PLANES, 81), NEUTRAL, np.uint16), lut_of(tau), k, limit,
                   min_plays)

    def copy(self):
        return MoveContextTable(self.counts, self.values, self.lut, self.k, self.limit, self.min_plays)

    def move_values(self):
        """Plane 81 as a MoveValueTable of its own (a copy): what bkt_move_value_update leaves on the same playouts."""
        return MoveValueTable(self.counts[:, 81], self.values[:, 81], self.lut, self.k, self.limit)

    def qualified(self):
        """The number of context entries (p < 81) whose played is at least min_plays."""
        return int((self.counts[:, :81, :, 0] >= self.min_plays).sum())

    def __getstate__(self):
        return dict(super().__getstate__(), min_plays=self.min_plays)

    def __setstate__(self, state):
        self.__init__(state["counts"], state["values"], state["lut"], state["k"], state["limit"], state["min_plays"])


def _values_of(table):
    values = table.values if isinstance(table, MoveContextTable) else np.asarray(table)
    if values.shape != (2, PLANES, 81) or values.dtype != np.uint16:
        raise ValueError("move-context values are uint16 [2, 82, 81]")
    return values


def move_context_weights(weights, values, colour, prev):
    """The weight rule for rows: weights [R,81] the weights w_in of the inner draw, values a MoveContextTable or uint16
    [2,82,81], colour int [R] the colour to move of each row (0 black, 1 white), prev int [R] the move played just before
    (anything outside 0..80 is plane 81) -> uint64 [R,81]: min(2^24 - 1, max(1, (w_in * values[colour, p, q]) >> 8))."""
    w = np.asarray(weights).astype(np.uint64)
    colour = np.asarray(colour, np.int64)
    v = _values_of(values)[colour, context_of(prev)].astype(np.uint64)
    return np.minimum(np.maximum((w * v) >> np.uint64(8), np.uint64(1)), np.uint64(WEIGHT_CAP))


def move_context_update_host(table, recs, moves, won, records, playouts):
    """bkt_move_context_update on the host: table a MoveContextTable, updated in place; recs uint8 [records,192], the
    starting records; moves int16 [records * playouts, max_plies] and won [records * playouts] as move_value_update_host
    takes them.  Every ply t of a row before the first entry <= MOVE_NONE whose move m is a board point adds a play to
    counts[c, 81, m], and to counts[c, p, m] when p = context_of(moves[row, t - 1]) (the record's last move at t == 0) is
    below 81, with c = (the record's colour to move) xor (t & 1), and a win when (won[row] != 0) == (t even); then every
    entry is halved until played < limit (limit > 0), and the values follow the module docstring's rule.
    -> the number of plays added (to plane 81)."""
    if not isinstance(table, MoveContextTable):
        raise TypeError("move_context_update_host updates a MoveContextTable in place")
    records, playouts = int(records), int(playouts)
    recs, moves, won = np.asarray(recs), np.asarray(moves), np.asarray(won).reshape(-1) != 0
    if records < 1 or playouts < 1 or moves.ndim != 2 or len(moves) != records * playouts or len(won) != len(moves) \
            or recs.shape != (records, L.POS_BYTES):
        raise ValueError(f"recs must be [{records}, {L.POS_BYTES}], moves [{records} * {playouts}, max_plies] and won "
                         f"[{records} * {playouts}]")
    if not 1 <= moves.shape[1] <= 1024 or playouts * moves.shape[1] >= 2 ** 31:
        raise ValueError("max_plies must be 1..1024 (BKT_MAX_PLAYOUT_PLIES) and playouts * max_plies below 2^31")
    m = moves.astype(np.int64)
    live = np.cumsum(m <= MOVE_NONE, 1) == 0
    point = live & (m >= 0) & (m <= 80)
    even = (np.arange(m.shape[1]) & 1) == 0
    c0 = np.repeat((L.record_turns(recs) & 1).astype(np.int64), playouts)
    c = c0[:, None] ^ (~even).astype(np.int64)[None, :]
    mover_won = won[:, None] == even[None, :]
    last = np.repeat(np.asarray(L.record_last_move(recs)).astype(np.int64), playouts)
    p = context_of(np.concatenate([last[:, None], m[:, :-1]], 1))
    mc = np.clip(m, 0, 80)
    counts, values = table.counts, table.values
    size = 2 * PLANES * 81
    for entry, mine in (((c * PLANES + 81) * 81 + mc, point), ((c * PLANES + p) * 81 + mc, point & (p < 81))):
        flat = entry[mine]
        counts[..., 0] += np.bincount(flat, minlength=size).reshape(2, PLANES, 81)
        counts[..., 1] += np.bincount(flat[mover_won[mine]], minlength=size).reshape(2, PLANES, 81)
    if table.limit > 0:
        while True:
            big = counts[..., 0] >= table.limit
            if not big.any():
                break
            counts[big] >>= 1
    idx = np.minimum(rate_index(counts[..., 0], counts[..., 1], table.k), 64)
    i1 = idx[:, 81:82]
    values[...] = table.lut[np.where(counts[..., 0] >= table.min_plays, (i1 + idx) >> 1, i1)]
    values[:, 81] = table.lut[idx[:, 81]]
    return int(point.sum())

"""The move-value table of the MAST playouts (the move-average sampling technique, Finnsson & Bjornsson 2008),
its host mirror and the two rules in numpy.  include/bokego_train.h has the definition the kernels, this module and the docs
share:

    counts int64 [2,81,2]   counts[c, m] = (played, won) of colour c (0 black, 1 white) on point m, over the playouts folded in
    values uint16 [2,81]    the factor of the draw's weight in units of 1/256: 256 neutral, every entry >= 1
    lut    uint16 [65]      the value of a win rate i / 64: lut_of(tau)[i] = rint(256 exp((i / 64 - 1 / 2) / tau)), clipped to
                            1..65535, so lut[32] == 256 whatever tau
    use     (move_value_weights)      w = min(2^24 - 1, max(1, (w_in * values[c, q]) >> 8)) on the weight w_in the pattern and
                                      tactics tables give a playable point q, c the colour to move
    update  (move_value_update_host)  every play of every playout counts for its colour and point, and wins with its mover;
                                      then, per entry: halved until played < limit (limit > 0), i = floor(64 (2 won + k) /
                                      (2 (played + k))), values = lut[i]

Everything is an integer: the device computes the same bits.  rollout.py's playouts take a MoveValueTable as move_values=
and update it in place; with rules="device" the live copies are tensors on the device (bkt_move_value_playouts reads
values, bkt_move_value_update writes counts and values) and `.counts` / `.values` download them when asked.

MoveValueTables is a table per game of a self-play batch: counts [count,2,81,2] and values [count,2,81] with one
lut, k and limit; slots= names the table of every row (bkt_move_value_playouts_tables) or record
(bkt_move_value_update_tables).  A slot outside 0..count-1 plays with neutral values and updates nothing, and a table that
no record names keeps every byte.
"""
import numpy as np

from . import lockstep as L

NEUTRAL = 256              # BKT_MOVE_VALUE_NEUTRAL
MAX_K = 65536              # BKT_MOVE_VALUE_MAX_K
MAX_LIMIT = 1 << 30        # BKT_MOVE_VALUE_MAX_LIMIT
MOVE_NONE = -2             # BKT_MOVE_NONE
WEIGHT_CAP = (1 << 24) - 1
MAX_TABLES = 4096          # BKT_MAX_MOVE_VALUE_TABLES
# the defaults of --playout-move-values: plausible and untuned
DEFAULT_TAU, DEFAULT_K, DEFAULT_LIMIT = 0.25, 16, 16384

__all__ = ["NEUTRAL", "MAX_K", "MAX_LIMIT", "MAX_TABLES", "DEFAULT_TAU", "DEFAULT_K", "DEFAULT_LIMIT", "MoveValueTable",
           "MoveValueTables", "lut_of", "check_tau", "check_k_limit", "rate_index", "move_value_weights", "move_value_update_host"]


def check_tau(tau):
    """tau as a float: finite and > 0 (ValueError)."""
    tau = float(tau)
    if not (tau > 0.0 and tau - tau == 0.0):
        raise ValueError(f"the temperature tau of a move-value table must be finite and > 0, got {tau}")
    return tau


def check_k_limit(k, limit):
    """(k, limit) as ints in the domain of bkt_move_value_update: 1 <= k <= MAX_K; limit == 0 or 2 <= limit <= MAX_LIMIT."""
    k, limit = int(k), int(limit)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k, the virtual plays of a move-value entry, must be 1..{MAX_K}, got {k}")
    if limit != 0 and not 2 <= limit <= MAX_LIMIT:
        raise ValueError(f"limit, the plays at which a move-value entry is halved, must be 0 (never) or 2..{MAX_LIMIT}, got {limit}")
    return k, limit


def lut_of(tau):
    """uint16 [65]: lut[i] = clip(rint(256 exp((i / 64 - 1 / 2) / tau)), 1, 65535), in float64 on the host, once."""
    tau = check_tau(tau)
    with np.errstate(over="ignore"):
        x = 256.0 * np.exp((np.arange(65, dtype=np.float64) / 64.0 - 0.5) / tau)
    return np.clip(np.rint(x), 1.0, 65535.0).astype(np.uint16)


def rate_index(played, won, k):
    """i = floor(64 (2 won + k) / (2 (played + k))), int64, elementwise: in 0..64 when 0 <= won <= played and k >= 1."""
    played, won = np.asarray(played, np.int64), np.asarray(won, np.int64)
    return (64 * (2 * won + int(k))) // (2 * (played + int(k)))


class MoveValueTable:
    """counts int64 [2,81,2], values uint16 [2,81], lut uint16 [65], k and limit (module docstring).  `.counts` and
    `.values` are the table on the host; device(dev) is a cached pair of tensors (counts, values) and the lut on dev that
    the device playouts read and update in place -- whichever side was written last is the table, and the other is brought
    up to date when it is asked for (`.counts` after a device update waits for that device), as replies.ReplyTable."""

    def __init__(self, counts, values, lut, k=DEFAULT_K, limit=DEFAULT_LIMIT):
        counts, values, lut = np.asarray(counts), np.asarray(values), np.asarray(lut)
        if counts.shape != (2, 81, 2) or counts.dtype != np.int64:
            raise ValueError(f"the counts of a move-value table are int64 [2, 81, 2], got {counts.dtype} {counts.shape}")
        if values.shape != (2, 81) or values.dtype != np.uint16 or (values < 1).any():
            raise ValueError(f"the values of a move-value table are uint16 [2, 81], every entry >= 1, got {values.dtype} {values.shape}")
        if lut.shape != (65,) or lut.dtype != np.uint16 or (lut < 1).any():
            raise ValueError(f"the lut of a move-value table is uint16 [65], every entry >= 1, got {lut.dtype} {lut.shape}")
        if (counts < 0).any() or (counts[..., 1] > counts[..., 0]).any():
            raise ValueError("the counts of a move-value table are 0 <= won <= played")
        self.k, self.limit = check_k_limit(k, limit)
        self._counts = np.array(counts, np.int64, order="C")
        self._values = np.array(values, np.uint16, order="C")
        self.lut = np.array(lut, np.uint16, order="C")
        self.lut.setflags(write=False)
        self._device = {}
        self._live = None                                             # the device whose tensors are newer than the arrays

    @classmethod
    def empty(cls, tau=DEFAULT_TAU, k=DEFAULT_K, limit=DEFAULT_LIMIT):
        """No play counted, every value lut_of(tau)[32] == 256."""
        return cls(np.zeros((2, 81, 2), np.int64), np.full((2, 81), NEUTRAL, np.uint16), lut_of(tau), k, limit)

    def _download(self):
        if self._live is not None:
            counts, values, _ = self._device[self._live]
            self._counts[...] = counts.cpu().numpy()
            self._values[...] = values.cpu().numpy().view(np.uint16)
            self._live = None                                         # the caller may write to the arrays: upload them next time

    @property
    def counts(self):
        self._download()
        return self._counts

    @property
    def values(self):
        self._download()
        return self._values

    def copy(self):
        return MoveValueTable(self.counts, self.values, self.lut, self.k, self.limit)

    def clear(self):
        """No play counted and every value neutral again (lut[32]), in place: what a new game starts with."""
        self.counts[...] = 0
        self.values[...] = self.lut[32]

    def occupancy(self):
        """The number of entries with at least one play."""
        return int((self.counts[..., 0] > 0).sum())

    def device(self, dev):
        """(counts int64 [2,81,2], values int16 [2,81] -- the bits of the uint16 entries -- , lut int16 [65]) on dev, the
        table itself from here on: what _trainlib.move_value_playouts reads and move_value_update writes."""
        import torch
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._live != dev:
            counts = torch.from_numpy(self.counts.copy())             # (.counts: first down from another device, if any)
            values = torch.from_numpy(self._values.view(np.int16).copy())
            if dev in self._device:
                self._device[dev][0].copy_(counts)
                self._device[dev][1].copy_(values)
            else:
                self._device[dev] = (counts.to(dev), values.to(dev), torch.from_numpy(self.lut.view(np.int16).copy()).to(dev))
            self._live = dev
        return self._device[dev]

    def __deepcopy__(self, memo):
        return self.copy()

    def __getstate__(self):
        return {"counts": self.counts.copy(), "values": self.values.copy(), "lut": np.array(self.lut), "k": self.k,
                "limit": self.limit}

    def __setstate__(self, state):
        self.__init__(state["counts"], state["values"], state["lut"], state["k"], state["limit"])


class MoveValueTables(MoveValueTable):
    """A move-value table per game of a batch: counts int64 [count,2,81,2] and values uint16 [count,2,81], with
    one lut uint16 [65], one k and one limit for all of them; created empty (no play counted, every value 256).  slots= of
    rollout.py's playouts names the table of every record.  `.counts`, `.values`, device(dev), clear(), deepcopy, pickle and
    the host/device liveness rule are MoveValueTable's; occupancy() is per table, and table(i) a MoveValueTable copy of
    table i."""

    def __init__(self, count, tau=DEFAULT_TAU, k=DEFAULT_K, limit=DEFAULT_LIMIT):
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)):
            raise TypeError(f"the number of move-value tables must be an int, got {type(count).__name__}")
        if not 1 <= count <= MAX_TABLES:
            raise ValueError(f"the number of move-value tables must be 1..{MAX_TABLES}, got {count}")
        self._set(np.zeros((int(count), 2, 81, 2), np.int64), np.full((int(count), 2, 81), NEUTRAL, np.uint16), lut_of(tau), k, limit)

    def _set(self, counts, values, lut, k, limit):
        self.k, self.limit = check_k_limit(k, limit)
        self._counts = np.array(counts, np.int64, order="C")
        self._values = np.array(values, np.uint16, order="C")
        self.lut = np.array(lut, np.uint16, order="C")
        self.lut.setflags(write=False)
        self._device = {}
        self._live = None

    @classmethod
    def empty(cls, count=1, tau=DEFAULT_TAU, k=DEFAULT_K, limit=DEFAULT_LIMIT):
        return cls(count, tau, k, limit)

    @property
    def count(self):
        return len(self._counts)

    def copy(self):
        new = object.__new__(MoveValueTables)
        new._set(self.counts, self.values, self.lut, self.k, self.limit)
        return new

    def occupancy(self):
        """int64 [count]: the number of entries of each table with at least one play."""
        return (self.counts[..., 0] > 0).sum((1, 2)).astype(np.int64)

    def table(self, i):
        """Table i as a MoveValueTable of its own (a copy)."""
        i = int(i)
        if not 0 <= i < self.count:
            raise IndexError(f"table {i} of {self.count}")
        return MoveValueTable(self.counts[i], self.values[i], self.lut, self.k, self.limit)

    def __setstate__(self, state):
        self._set(state["counts"], state["values"], state["lut"], state["k"], state["limit"])


def _values_of(table):
    values = table.values if isinstance(table, MoveValueTable) else np.asarray(table)
    if values.shape[-2:] != (2, 81) or values.ndim not in (2, 3) or values.dtype != np.uint16:
        raise ValueError("move values are uint16 [2, 81], or with slots [count, 2, 81]")
    return values


def _rows_values(values, slots, rows):
    """uint16 [rows,2,81]: the values of every row -- the one table's without slots, else table slots[row]'s, and 256
    everywhere for a slot outside 0..count-1 (compared before it indexes)."""
    if slots is None:
        if values.ndim != 2:
            raise TypeError("move-value tables need slots: the table of every row")
        return np.broadcast_to(values, (rows, 2, 81))
    if values.ndim != 3:
        raise TypeError("slots name the table of every row among many move-value tables: not with a single table")
    slots = np.asarray(slots, np.int64)
    if slots.shape != (rows,):
        raise ValueError(f"slots must be an int array of one entry per row, [{rows}]")
    ok = (slots >= 0) & (slots < len(values))
    out = values[np.where(ok, slots, 0)]
    out[~ok] = NEUTRAL
    return out


def move_value_weights(weights, values, colour, slots=None):
    """The weight rule for rows: weights [R,81] the weights w_in of the inner draw (rollout.move_weights_host's on the
    playable points; anything elsewhere), values a MoveValueTable or uint16 [2,81], colour int [R] the colour to move of
    each row (0 black, 1 white) -> uint64 [R,81]: min(2^24 - 1, max(1, (w_in * values[colour, q]) >> 8)).  With slots int
    [R], values is a MoveValueTables or uint16 [count,2,81] and row r uses table slots[r] (a slot out of range: 256)."""
    w = np.asarray(weights).astype(np.uint64)
    colour = np.asarray(colour, np.int64)
    v = _rows_values(_values_of(values), slots, len(w))[np.arange(len(w)), colour].astype(np.uint64)
    return np.minimum(np.maximum((w * v) >> np.uint64(8), np.uint64(1)), np.uint64(WEIGHT_CAP))


def move_value_update_host(table, recs, moves, won, records, playouts, slots=None):
    """bkt_move_value_update on the host: table a MoveValueTable, updated in place; recs uint8 [records,192], the starting
    records; moves int16 [records * playouts, max_plies] and won [records * playouts] as reply_update_host takes them.
    Every ply t of a row before the first entry <= MOVE_NONE whose move m is a board point adds a play to
    counts[c, m] with c = (the record's colour to move) xor (t & 1), and a win when (won[row] != 0) == (t even); then every
    entry is halved until played < limit (limit > 0), and values = lut[rate_index(played, won, k)].
    With slots int [records], table is a MoveValueTables (bkt_move_value_update_tables): the rule applies per table, over the
    records whose slot names it; a table that no record names keeps every byte, and a slot outside 0..count-1 updates
    nothing.
    -> the number of plays added."""
    many = isinstance(table, MoveValueTables)
    if not isinstance(table, MoveValueTable):
        raise TypeError("move_value_update_host updates a MoveValueTable or a MoveValueTables in place")
    if many != (slots is not None):
        raise TypeError("slots name the table of every record among many move-value tables: required with a MoveValueTables, "
                        "refused with a MoveValueTable")
    records, playouts = int(records), int(playouts)
    recs, moves, won = np.asarray(recs), np.asarray(moves), np.asarray(won).reshape(-1) != 0
    if records < 1 or playouts < 1 or moves.ndim != 2 or len(moves) != records * playouts or len(won) != len(moves) \
            or recs.shape != (records, L.POS_BYTES):
        raise ValueError(f"recs must be [{records}, {L.POS_BYTES}], moves [{records} * {playouts}, max_plies] and won "
                         f"[{records} * {playouts}]")
    if not 1 <= moves.shape[1] <= 1024 or playouts * moves.shape[1] >= 2 ** 31:
        raise ValueError("max_plies must be 1..1024 (BKT_MAX_PLAYOUT_PLIES) and playouts * max_plies below 2^31")
    if many:
        slots = np.asarray(slots)
        if slots.shape != (records,) or slots.dtype.kind not in "iu":
            raise ValueError(f"slots must be an int array of one entry per record, [{records}]")
        slots = slots.astype(np.int64)
    m = moves.astype(np.int64)
    live = np.cumsum(m <= MOVE_NONE, 1) == 0
    point = live & (m >= 0) & (m <= 80)
    even = (np.arange(m.shape[1]) & 1) == 0
    c0 = np.repeat((L.record_turns(recs) & 1).astype(np.int64), playouts)
    c = c0[:, None] ^ (~even).astype(np.int64)[None, :]
    mover_won = won[:, None] == even[None, :]
    entry = c * 81 + np.clip(m, 0, 80)
    all_counts, all_values = (table.counts, table.values) if many else (table.counts[None], table.values[None])
    added = 0
    for t in (np.unique(slots[(slots >= 0) & (slots < table.count)]) if many else (0,)):
        mine = point if not many else point & np.repeat(slots == t, playouts)[:, None]
        flat = entry[mine]
        counts = all_counts[t]
        counts[..., 0] += np.bincount(flat, minlength=162).reshape(2, 81)
        counts[..., 1] += np.bincount(flat[mover_won[mine]], minlength=162).reshape(2, 81)
        if table.limit > 0:
            while True:
                big = counts[..., 0] >= table.limit
                if not big.any():
                    break
                counts[big] >>= 1
        all_values[t][...] = table.lut[np.minimum(rate_index(counts[..., 0], counts[..., 1], table.k), 64)]
        added += int(mine.sum())
    return added

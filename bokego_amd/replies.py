"""The last-good-reply table of the playouts (LGRF-1: Drake 2009, Baier & Drake 2010), its host mirror and the
two rules in numpy.  include/bokego_train.h has the definition the kernels, this module and the docs share:

    replies uint8 [2,81]    replies[c, prev]: the reply of colour c (0 black, 1 white) to the opponent's move on the board
                            point prev; 0..80 a point, NONE = 255 none, any other value above 80 treated as none
    use       (reply_moves)        in a playout, the side to move plays replies[c, last move] when that is a point of the
                                   playable set; otherwise the playout's own draw decides
    update    (reply_update_host)  after a batch of playouts, rows and plies in ascending order: the winner's replies are
                                   stored, the loser's are taken out where the table still holds them

rollout.py's playouts take a ReplyTable as replies= and update it in place; with rules="device" the live copy is a tensor
on the device (bkt_reply_playouts reads it, bkt_reply_update writes it) and `.array` downloads it when asked.

ReplyTables(count) is `count` such tables in one array, a table per game of a self-play batch: the playouts and
the update then take `slots`, the table of every row (of every record): the single-table rules applied, per slot, to that
slot's rows in order.  A slot outside 0..count-1 plays as an empty table and updates nothing.

ReplyTable2 is the table keyed by the last two moves (LGRF-2; the header has its definition too):

    replies2 uint8 [2,82,81]  replies2[c, p2, p1], p2 < 81: the reply of colour c to the opponent's move on p1 that followed
                              c's own move on p2; plane p2 == 81 is the table above, replies2[c, 81, p1] = replies[c, p1]
    use       (reply2_moves)        the pair entry when p1 and p2 are board points and its point is playable; else the single
                                    entry (plane 81) likewise; else the playout's own draw
    update    (reply2_update_host)  the fold above, applied at every event to [c, 81, p1] and, when p2 is a board point, to
                                    [c, p2, p1]

ReplyTables2(count) is `count` pair tables in one array, a pair table per game of a self-play batch, with `slots`
exactly as a ReplyTables takes them: reply2_moves and reply2_update_host are then the single-table rules applied, per slot,
to that slot's rows in order.
"""
import numpy as np

from . import lockstep as L

NONE = 255                 # BKT_REPLY_NONE
MOVE_NONE = -2             # BKT_MOVE_NONE

__all__ = ["NONE", "ReplyTable", "ReplyTable2", "ReplyTables", "ReplyTables2", "reply_moves", "reply_update_host", "reply2_moves",
           "reply2_plies_of", "reply2_update_host"]


class ReplyTable:
    """uint8 [2,81] replies (module docstring).  `.array` is the table on the host; device(dev) is a cached tensor on dev
    that the device playouts read and update in place -- whichever was written last is the table, and the other is brought
    up to date when it is asked for (`.array` after a device update waits for that device)."""

    def __init__(self, array, shape=(2, 81)):
        array = np.asarray(array)
        if array.shape != shape or array.dtype != np.uint8:
            raise ValueError(f"a reply table is uint8 [2, 81]: expected uint8 {list(shape)}, got {array.dtype} {array.shape}")
        self._array = np.array(array, np.uint8, order="C")
        self._device = {}
        self._live = None                                             # the device whose tensor is newer than _array

    @classmethod
    def empty(cls):
        return cls(np.full((2, 81), NONE, np.uint8))

    @property
    def array(self):
        if self._live is not None:
            self._array[...] = self._device[self._live].cpu().numpy()
            self._live = None                                         # the caller may write to the array: upload it next time
        return self._array

    def copy(self):
        return ReplyTable(self.array)

    def clear(self):
        """Every entry NONE, in place."""
        self.array[...] = NONE

    def occupancy(self):
        """The number of entries that hold a point."""
        return int((self.array <= 80).sum())

    def device(self, dev):
        """uint8 [2,81] on dev, the table itself from here on: what _trainlib.reply_playouts reads and reply_update writes."""
        import torch
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._live != dev:
            host = torch.from_numpy(self.array.copy())                # (.array: first down from another device, if any)
            if dev in self._device:
                self._device[dev].copy_(host)
            else:
                self._device[dev] = host.to(dev)
            self._live = dev
        return self._device[dev]

    def __deepcopy__(self, memo):
        return self.copy()

    def __getstate__(self):
        return {"array": self.array.copy()}

    def __setstate__(self, state):
        self.__init__(state["array"])


class ReplyTables(ReplyTable):
    """uint8 [count,2,81]: `count` reply tables, table i for the rows whose slot is i.  `.array`, device(dev), clear() and
    the caching contract are ReplyTable's; occupancy() is per table, and table(i) a ReplyTable copy of table i."""

    def __init__(self, count, array=None):
        count = int(count)
        if not 1 <= count <= 65536:
            raise ValueError("the number of reply tables must be 1..65536 (BKT_MAX_BATCH)")
        super().__init__(np.full((count, 2, 81), NONE, np.uint8) if array is None else array, (count, 2, 81))
        self.count = count

    @classmethod
    def empty(cls, count=1):
        return cls(count)

    def copy(self):
        return ReplyTables(self.count, self.array)

    def occupancy(self):
        """int64 [count]: the number of entries of each table that hold a point."""
        return (self.array <= 80).sum((1, 2)).astype(np.int64)

    def table(self, i):
        return ReplyTable(self.array[int(i)])

    def __getstate__(self):
        return {"count": self.count, "array": self.array.copy()}

    def __setstate__(self, state):
        self.__init__(state["count"], state["array"])


class ReplyTable2(ReplyTable):
    """uint8 [2,82,81]: the replies keyed by the last two moves, plane 81 the single-move table (module docstring).
    `.array`, device(dev), clear(), occupancy() (over all planes) and the caching contract are ReplyTable's; singles() is a
    ReplyTable copy of plane 81 and pairs_occupancy() the entries of planes 0..80 that hold a point."""

    SHAPE = (2, 82, 81)

    def __init__(self, array):
        array = np.asarray(array)
        if array.shape != self.SHAPE or array.dtype != np.uint8:
            raise ValueError(f"a pair reply table is uint8 [2, 82, 81], got {array.dtype} {array.shape}")
        super().__init__(array, self.SHAPE)

    @classmethod
    def empty(cls):
        return cls(np.full(cls.SHAPE, NONE, np.uint8))

    def copy(self):
        return ReplyTable2(self.array)

    def singles(self):
        return ReplyTable(self.array[:, 81])

    def pairs_occupancy(self):
        return int((self.array[:, :81] <= 80).sum())


class ReplyTables2(ReplyTable):
    """uint8 [count,2,82,81]: `count` pair reply tables, table i for the rows whose slot is i.  `.array`, device(dev),
    clear() and the caching contract are ReplyTable's; occupancy() and pairs_occupancy() are per table, table(i) is a
    ReplyTable2 copy of table i and singles() a ReplyTables copy of the plane-81s."""

    MAX = 4096                                                        # BKT_MAX_REPLY2_TABLES

    def __init__(self, count, array=None):
        count = int(count)
        if not 1 <= count <= self.MAX:
            raise ValueError(f"the number of pair reply tables must be 1..{self.MAX} (BKT_MAX_REPLY2_TABLES)")
        shape = (count,) + ReplyTable2.SHAPE
        array = np.full(shape, NONE, np.uint8) if array is None else np.asarray(array)
        if array.shape != shape or array.dtype != np.uint8:
            raise ValueError(f"pair reply tables are uint8 [count, 2, 82, 81]: expected {list(shape)}, got {array.dtype} {array.shape}")
        super().__init__(array, shape)
        self.count = count

    @classmethod
    def empty(cls, count=1):
        return cls(count)

    def copy(self):
        return ReplyTables2(self.count, self.array)

    def occupancy(self):
        """int64 [count]: the number of entries of each table, over all planes, that hold a point."""
        return (self.array <= 80).sum((1, 2, 3)).astype(np.int64)

    def pairs_occupancy(self):
        """int64 [count]: the entries of planes 0..80 of each table that hold a point."""
        return (self.array[:, :, :81] <= 80).sum((1, 2, 3)).astype(np.int64)

    def table(self, i):
        return ReplyTable2(self.array[int(i)])

    def singles(self):
        return ReplyTables(self.count, self.array[:, :, 81])

    def __getstate__(self):
        return {"count": self.count, "array": self.array.copy()}

    def __setstate__(self, state):
        self.__init__(state["count"], state["array"])


def _host_array(table):
    return table.array if isinstance(table, ReplyTable) else np.asarray(table)


def slots_of(table, slots, n, what="record"):
    """The one check of slots: for n rows (records) of many tables -- a ReplyTables or an array [count,2,81], a ReplyTables2
    or an array [count,2,82,81] -- an int array [n] -> int64 [n]; with a single table (a ReplyTable, a ReplyTable2 or an
    array [2,81]) or none at all, slots must be None -> None.  It looks at the kind of `table` only, never at its entries:
    a table that lives on a device stays there."""
    many = isinstance(table, (ReplyTables, ReplyTables2)) or (
        table is not None and not isinstance(table, ReplyTable) and np.ndim(table) in (3, 4))
    if not many:
        if slots is not None:
            raise TypeError("slots name the table of every record among many reply tables: not with a single table or without one")
        return None
    if slots is None:
        raise TypeError(f"reply tables need slots: the table of every {what}")
    slots = np.asarray(slots)
    if slots.shape != (n,) or slots.dtype.kind not in "iu":
        raise ValueError(f"slots must be an int array of one entry per {what}, [{n}]")
    return slots.astype(np.int64)


def _tables_and_slots(t, slots, n, what):
    """The array t and its checked slots, a single table read as [1,2,81] (a view) with every slot 0
    -> (tables [count,2,81], slots int64 [n])."""
    slots = slots_of(t, slots, n, what)
    return (t[None], np.zeros(n, np.int64)) if slots is None else (t, slots)


def reply_moves(table, recs, playable, slots=None):
    """The use rule for rows: recs uint8 [R,192], playable bool [R,81] -> int64 [R]: the reply the table makes the side to
    move play, or -1 where it decides nothing (the last move is no board point, the entry is no point, or the point is
    not playable).  An entry is compared before it indexes.  With tables [count,2,81], slots [R] names each row's table;
    a slot outside 0..count-1 is compared before it indexes, and such a row has no reply."""
    t, slots = _tables_and_slots(_host_array(table), slots, len(recs), "row")
    lm = L.record_last_move(recs).astype(np.int64)
    c = (L.record_turns(recs) & 1).astype(np.int64)
    asks = (lm >= 0) & (lm <= 80) & (slots >= 0) & (slots < len(t))   # the row has a table and a move to reply to
    r = np.where(asks, t[np.where(asks, slots, 0), c, np.where(asks, lm, 0)], NONE).astype(np.int64)
    ok = (r <= 80) & np.asarray(playable)[np.arange(len(recs)), np.minimum(r, 80)]
    return np.where(ok, r, -1)


def reply_plies_of(table, recs, moves, playouts):
    """The plies of finished playouts that `table` (as it stood while they ran) decided, counted from their history: recs
    uint8 [records,192] the starting records, moves int16 [records * playouts, L].  A playable reply is always played and
    a played move was playable, so the table decided ply t exactly when moves[row, t] is its reply to the move before."""
    t = _host_array(table)
    moves = np.asarray(moves).astype(np.int64)
    lm0 = np.repeat(L.record_last_move(recs).astype(np.int64), playouts)
    c0 = np.repeat((L.record_turns(recs) & 1).astype(np.int64), playouts)
    prev = np.concatenate([lm0[:, None], moves[:, :-1]], 1)
    live = np.cumsum(moves <= MOVE_NONE, 1) == 0
    c = c0[:, None] ^ (np.arange(moves.shape[1]) & 1)[None, :]
    ok = live & (moves >= 0) & (moves <= 80) & (prev >= 0) & (prev <= 80)
    return int((ok & (t[c, np.clip(prev, 0, 80)] == moves)).sum())


def reply_update_host(table, recs, moves, won, records, playouts, slots=None):
    """bkt_reply_update on the host, the sequential fold itself: table a ReplyTable (or a uint8 [2,81] array), updated in
    place; recs uint8 [records,192], the starting records; moves int16 [records * playouts, max_plies] and won
    [records * playouts] as amaf_counts_sides_host takes them.  Rows ascending, plies ascending up to the first entry
    <= MOVE_NONE: with c the mover's colour ((turn of the record + t) & 1), prev the record's last move at t = 0 and
    moves[row, t - 1] after it, m = moves[row, t] -- when both are board points, a mover who won the row stores
    table[c, prev] = m, and one who lost clears the entry if it holds m.
    With tables [count,2,81] (a ReplyTables), slots [records] names each record's table: table i is folded with the records
    whose slot is i, in ascending order; a record whose slot is outside 0..count-1 updates nothing (and counts no event).
    -> (set, cleared, nothing): the events that stored, that cleared, and that did neither."""
    tables = _host_array(table)
    records, playouts = int(records), int(playouts)
    recs, moves, won = np.asarray(recs), np.asarray(moves), np.asarray(won).reshape(-1) != 0
    if records < 1 or playouts < 1 or moves.ndim != 2 or len(moves) != records * playouts or len(won) != len(moves) \
            or recs.shape != (records, L.POS_BYTES):
        raise ValueError(f"recs must be [{records}, {L.POS_BYTES}], moves [{records} * {playouts}, max_plies] and won "
                         f"[{records} * {playouts}]")
    if tables.shape[-2:] != (2, 81) or tables.ndim not in (2, 3) or tables.dtype != np.uint8:
        raise ValueError("a reply table is uint8 [2, 81], reply tables uint8 [count, 2, 81]")
    tables, slots = _tables_and_slots(tables, slots, records, "record")
    lm0 = L.record_last_move(recs).astype(np.int64)
    c0 = (L.record_turns(recs) & 1).astype(np.int64)
    n_set = n_cleared = n_nothing = 0
    for row in range(len(moves)):
        r = row // playouts
        if not 0 <= slots[r] < len(tables):
            continue
        t, prev, win = tables[slots[r]], int(lm0[r]), bool(won[row])
        for k, m in enumerate(moves[row].tolist()):
            if m <= MOVE_NONE:
                break
            if 0 <= m <= 80 and 0 <= prev <= 80:
                c = int(c0[r]) ^ (k & 1)
                if win == (k % 2 == 0):
                    t[c, prev] = m
                    n_set += 1
                elif t[c, prev] == m:
                    t[c, prev] = NONE
                    n_cleared += 1
                else:
                    n_nothing += 1
            prev = m
    return n_set, n_cleared, n_nothing


def _tables2_and_slots(t, slots, n, what):
    """_tables_and_slots for pair tables: a single table [2,82,81] read as [1,2,82,81] (a view) with every slot 0
    -> (tables [count,2,82,81], slots int64 [n])."""
    if t.ndim == 3:
        if slots is not None:
            raise TypeError("slots name the table of every record among many reply tables: not with a single table or without one")
        return t[None], np.zeros(n, np.int64)
    return t, slots_of(t, slots, n, what)


def reply2_moves(table, recs, prev2, playable, slots=None):
    """The use rule of a pair table for rows: table a ReplyTable2 (or uint8 [2,82,81]), recs uint8 [R,192], prev2 int [R]
    the move played two plies ago in each row's playout (anything outside 0..80 where there is none or it was a pass),
    playable bool [R,81] -> (move int64 [R], which int64 [R]): the reply the table makes the side to move play, or -1 where
    it decides nothing, and which lookup decided -- 2 the pair entry, 1 the single entry (plane 81), 0 neither.  Entries and
    moves are compared before they index.  With tables [count,2,82,81] (a ReplyTables2), slots [R] names each row's table;
    a slot outside 0..count-1 is compared before it indexes, and such a row has no reply."""
    t, slots = _tables2_and_slots(_host_array(table), slots, len(recs), "row")
    playable = np.asarray(playable)
    rows = np.arange(len(recs))
    p1 = L.record_last_move(recs).astype(np.int64)
    p2 = np.asarray(prev2).astype(np.int64)
    c = (L.record_turns(recs) & 1).astype(np.int64)
    has = (slots >= 0) & (slots < len(t))
    of = np.where(has, slots, 0)
    asks = has & (p1 >= 0) & (p1 <= 80)
    pair = asks & (p2 >= 0) & (p2 <= 80)
    at = np.where(asks, p1, 0)
    r2 = np.where(pair, t[of, c, np.where(pair, p2, 81), at], NONE).astype(np.int64)
    r1 = np.where(asks, t[of, c, 81, at], NONE).astype(np.int64)
    ok2 = (r2 <= 80) & playable[rows, np.minimum(r2, 80)]
    ok1 = (r1 <= 80) & playable[rows, np.minimum(r1, 80)]
    return np.where(ok2, r2, np.where(ok1, r1, -1)), np.where(ok2, 2, np.where(ok1, 1, 0))


def reply2_plies_of(table, recs, moves, playouts):
    """reply_plies_of for a pair table -> (pair plies, single plies): the plies of finished playouts that the pair entries
    of `table` (as it stood while they ran) decided, and those its plane 81 decided.  A playable reply is always played and
    a played move was playable, so the pair entry decided ply t exactly when moves[row, t] equals it, and plane 81 did
    when the pair entry did not and moves[row, t] equals the single entry."""
    t = _host_array(table)
    moves = np.asarray(moves).astype(np.int64)
    lm0 = np.repeat(L.record_last_move(recs).astype(np.int64), playouts)
    c0 = np.repeat((L.record_turns(recs) & 1).astype(np.int64), playouts)
    p1 = np.concatenate([lm0[:, None], moves[:, :-1]], 1)
    p2 = np.concatenate([np.full((len(moves), 1), MOVE_NONE, np.int64), p1[:, :-1]], 1)
    live = np.cumsum(moves <= MOVE_NONE, 1) == 0
    c = c0[:, None] ^ (np.arange(moves.shape[1]) & 1)[None, :]
    ok = live & (moves >= 0) & (moves <= 80) & (p1 >= 0) & (p1 <= 80)
    has2 = ok & (p2 >= 0) & (p2 <= 80)
    at = np.clip(p1, 0, 80)
    by_pair = has2 & (t[c, np.clip(p2, 0, 80), at] == moves)
    by_single = ok & ~by_pair & (t[c, 81, at] == moves)
    return int(by_pair.sum()), int(by_single.sum())


def reply2_update_host(table, recs, moves, won, records, playouts, slots=None):
    """bkt_reply2_update on the host, the sequential fold itself: table a ReplyTable2 (or a uint8 [2,82,81] array), updated
    in place; the other arguments as reply_update_host takes them.  Rows ascending, plies ascending up to the first entry
    <= MOVE_NONE: with c the mover's colour, p1 the move before (the record's last move at t = 0), p2 the move before that
    (the record's last move at t = 1, none at t = 0) and m = moves[row, t] -- when m and p1 are board points, the fold of
    reply_update_host is applied to table[c, 81, p1] and, when p2 is a board point, to table[c, p2, p1].
    With tables [count,2,82,81] (a ReplyTables2), slots [records] names each record's table: table i is folded with the
    records whose slot is i, in ascending order; a record whose slot is outside 0..count-1 updates nothing.
    -> (set, cleared, nothing): the entries touched that were stored, that were cleared, and that stayed."""
    tables = _host_array(table)
    records, playouts = int(records), int(playouts)
    recs, moves, won = np.asarray(recs), np.asarray(moves), np.asarray(won).reshape(-1) != 0
    if records < 1 or playouts < 1 or moves.ndim != 2 or len(moves) != records * playouts or len(won) != len(moves) \
            or recs.shape != (records, L.POS_BYTES):
        raise ValueError(f"recs must be [{records}, {L.POS_BYTES}], moves [{records} * {playouts}, max_plies] and won "
                         f"[{records} * {playouts}]")
    if tables.shape[-3:] != (2, 82, 81) or tables.ndim not in (3, 4) or tables.dtype != np.uint8:
        raise ValueError("a pair reply table is uint8 [2, 82, 81], pair reply tables uint8 [count, 2, 82, 81]")
    tables, slots = _tables2_and_slots(tables, slots, records, "record")
    lm0 = L.record_last_move(recs).astype(np.int64)
    c0 = (L.record_turns(recs) & 1).astype(np.int64)
    counts = [0, 0, 0]
    for row in range(len(moves)):
        r = row // playouts
        if not 0 <= slots[r] < len(tables):
            continue
        t, p1, p2, win = tables[slots[r]], int(lm0[r]), None, bool(won[row])
        for k, m in enumerate(moves[row].tolist()):
            if m <= MOVE_NONE:
                break
            if 0 <= m <= 80 and 0 <= p1 <= 80:
                c = int(c0[r]) ^ (k & 1)
                for plane in (81,) + ((p2,) if p2 is not None and 0 <= p2 <= 80 else ()):
                    if win == (k % 2 == 0):
                        t[c, plane, p1] = m
                        counts[0] += 1
                    elif t[c, plane, p1] == m:
                        t[c, plane, p1] = NONE
                        counts[1] += 1
                    else:
                        counts[2] += 1
            p1, p2 = m, p1
    return tuple(counts)

"""What the lock-step playout drivers (reinforce.play_games, genvals.generate, rollout) share; DESIGN 15.

The host mirrors of the device sampler (Philox4x32-10, the float64 CDF), the host rules behind every rules="host"
path (bk_pos_play, bk_features_batch_u8, bk_pos_area_score), the fields of a bk_pos record read from a numpy array or
from a tensor, the Philox counter layout (g mod 2^32, word 1, g >> 32, stream) with its table of streams, the logits of
row slices through their engines, phase timing, and the argument checks.  The drivers call the host rules through this
module (L.play_host, L.features_batch), and the helpers here look _play_fn and features_batch up at call time, so a
patch on this module's names bites in every driver.
"""
import ctypes
import time

import numpy as np
import torch

from . import go
from ._trainlib import seed_u64  # noqa: F401  (the drivers' seed -> key; one definition, beside the binding that needs it)

KOMI = 5.5
LEGAL_PLANE = 5            # nnet.features' "legal" plane (reference nnet.py:198)
POS_BYTES = 192            # sizeof(bk_pos)
PLANE_BYTES = 27 * 81

# ---- Philox4x32-10 and the sampler, host mirrors of bk_train.hip (float64) ----------------------------------------------
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32 [..., 4], key uint32 [..., 2] (broadcast) -> uint32 [..., 4] (Random123's philox4x32 with 10 rounds)."""
    c = [np.asarray(ctr, np.uint64)[..., i] & _MASK32 for i in range(4)]
    k = np.asarray(key, np.uint64)
    k0, k1 = k[..., 0] & _MASK32, k[..., 1] & _MASK32
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(PHILOX_W[0])) & _MASK32
            k1 = (k1 + np.uint64(PHILOX_W[1])) & _MASK32
        p0 = np.uint64(PHILOX_M[0]) * c[0]
        p1 = np.uint64(PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK32]
    return np.stack(c, -1).astype(np.uint32)


def seed_key(seed):
    """--seed (an unsigned 64-bit integer) -> the Philox key words (low, high)."""
    s = seed_u64(seed)
    return np.array([s & 0xFFFFFFFF, s >> 32], np.uint32)


def uniform(x0):
    """The first Philox output word -> u = (x0 >> 8) * 2^-24 in [0, 1), exact in float32 and float64."""
    return (np.asarray(x0, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def sample_host(logits, legal, u):
    """bkt_sample_moves in float64: logits [B,81], legal bool [B,81], u [B] -> (moves int32 [B], logp float64 [B]).
    The move is the first point whose inclusive prefix of p = exp(x - max) exceeds u * sum p; an illegal sample becomes
    the legal point of the largest logit (lowest index on ties); -1 when no point is legal.
    A degenerate row (degenerate_rows) makes no draw: its move is that replacement with NaN ordered as -inf, whatever u
    is, and its logp is NaN (bokego_train.h)."""
    with np.errstate(invalid="ignore"):                              # widening a signalling NaN raises the flag
        raw = np.asarray(logits, np.float64)
    legal = np.asarray(legal, bool)
    deg = degenerate_rows(raw)
    x = np.where(np.isnan(raw), -np.inf, raw)
    xo = np.where(deg[:, None], 0.0, x)                              # the draw of an ordinary row; a degenerate one's is unused
    m = xo.max(1, keepdims=True)
    c = np.cumsum(np.exp(xo - m), 1)
    S = c[:, -1]
    mv = np.argmax(c > (np.asarray(u, np.float64) * S)[:, None], 1)
    rows = np.arange(len(x))
    bad = deg | ~legal[rows, mv]
    best = np.where(legal, x, -np.inf)
    fix = np.argmax(legal & (best == best.max(1, keepdims=True)), 1)  # the lowest legal index also when every legal logit is -inf
    mv = np.where(bad, fix, mv)
    none = ~legal.any(1)
    mv[none] = -1
    logp = np.where(none, 0.0, xo[rows, np.maximum(mv, 0)] - m[:, 0] - np.log(S))
    return mv.astype(np.int32), np.where(deg, np.nan, logp)


def degenerate_rows(logits):
    """bool [B]: the rows bkt_sample_moves makes no draw on: a NaN or +inf logit, or all 81 at -inf."""
    x = np.asarray(logits)
    return np.isnan(x).any(1) | (x == np.inf).any(1) | (x == -np.inf).all(1)


def cdf_margin(logits, u):
    """min_i |u - CDF_i| over the float64 CDF of each row: how close u lies to a boundary between two points."""
    x = np.asarray(logits, np.float64)
    c = np.cumsum(np.exp(x - x.max(1, keepdims=True)), 1)
    c /= c[:, -1:]
    return np.abs(c - np.asarray(u, np.float64)[:, None]).min(1)


# ---- the counters (g mod 2^32, word 1, g >> 32, stream) --------------------------------------------------------------------
# Word 3 names the draw, so that no two of them share a counter for the same game g:
STREAM_MOVE = 0            # genvals: the move at ply p = word 1 (SL, random or RL, and finish_games running on from ply 90)
STREAM_R = 1               # genvals: r_g, the game's random ply (word 1 = 0)
STREAM_ROLLOUT = 2         # rollout.finish_games / random_playouts: word 1 = the record's turn + the plies played there
STREAM_VALUE = 3           # rollout.playout_value: g = the record's Zobrist hash, playout j has word 3 = 4 * j + 3


def value_streams(n):
    """Word 3 of the n playouts of playout_value: 4 * j + STREAM_VALUE, so streams 0..2 stay with the above."""
    return 4 * np.arange(n, dtype=np.uint32) + STREAM_VALUE


def game_counters(g, word1, stream):
    """The counter words (g mod 2^32, word1, g >> 32, stream) as int32 [N, 4] (the bits the kernels read as uint32);
    g (unsigned 64-bit), word1 and stream broadcast against each other, N = the size of the broadcast."""
    g, word1, stream = np.asarray(g, np.uint64), np.asarray(word1, np.int64), np.asarray(stream, np.int64)
    c = np.empty(np.broadcast_shapes(g.shape, word1.shape, stream.shape) + (4,), np.uint32)
    c[..., 0] = g & _MASK32
    c[..., 1] = word1.astype(np.uint32)
    c[..., 2] = g >> np.uint64(32)
    c[..., 3] = stream
    return c.reshape(-1, 4).view(np.int32)


def value_counters_device(recs, n):
    """game_counters(the hash of each record, 0, value_streams(n)) built on the device of recs (a uint8 [R,192] tensor)
    -> int32 [R * n, 4] there: no download and no wait."""
    h = record_hash_words(recs)
    c = torch.zeros((len(recs), n, 4), dtype=torch.int32, device=recs.device)
    c[:, :, 0] = h[:, :1]
    c[:, :, 2] = h[:, 1:]
    c[:, :, 3] = 4 * torch.arange(n, dtype=torch.int32, device=recs.device) + STREAM_VALUE
    return c.view(-1, 4)


# ---- the fields of bk_pos records, uint8 [n, 192]: a numpy array or a tensor (the result stays where the records are) -----
# byte offsets in struct bk_pos (include/bokego_go.h); the machine is little-endian
OFF_KO, OFF_LAST_MOVE, OFF_TURN, OFF_HASH = 164, 166, 172, 184        # int16, int16, int32, uint64


def _field(recs, off, dtype, words=1):
    """The `words` values of `dtype` (a numpy dtype name that torch has too) at byte `off` of every record -> [n, words]."""
    nbytes = words * np.dtype(dtype).itemsize
    if isinstance(recs, torch.Tensor):
        return recs[:, off:off + nbytes].contiguous().view(getattr(torch, dtype))
    return np.ascontiguousarray(recs[:, off:off + nbytes]).view(dtype)


def record_ko(recs):
    """int16 [n]: the ko point, or -1."""
    return _field(recs, OFF_KO, "int16")[:, 0]


def record_last_move(recs):
    """int16 [n]: the last move (go.PASS for a pass)."""
    return _field(recs, OFF_LAST_MOVE, "int16")[:, 0]


def record_turns(recs):
    """int32 [n]: the `turn` field (numpy: a copy, also of a single record, whose slice is contiguous as it lies)."""
    t = _field(recs, OFF_TURN, "int32")[:, 0]
    return t if isinstance(t, torch.Tensor) else t.copy()


def record_hash_words(recs):
    """int32 [n, 2]: the low and the high word of the Zobrist hash."""
    return _field(recs, OFF_HASH, "int32", 2)


def black_to_move(recs):
    """bool [n]: the turn is even (its low byte decides)."""
    return (recs[:, OFF_TURN] & 1) == 0


# ---- the host rules ----------------------------------------------------------------------------------------------------------
_PLAY = None


def _play_fn():
    """bk_pos_play taking a plain address (the records live in numpy arrays)."""
    global _PLAY
    if _PLAY is None:
        _PLAY = ctypes.cast(go.golib().bk_pos_play, ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int))
    return _PLAY


def pos_ptr(rec):
    """One record (a row of a numpy array) as the bk_pos * the host rules take."""
    return ctypes.cast(rec.ctypes.data, ctypes.POINTER(go.Pos))


def play_host(recs, rows, moves, describe, liberties=False):
    """bk_pos_play(moves[k]) on record rows[k] of recs (C-contiguous uint8 [n,192], in place; -1 plays a pass).  A move
    the rules refuse raises RuntimeError(describe(row, move)), the caller's wording of which row or game it was.
    liberties: bk_pos_liberties after every move, so that the record carries its liberty cache as the device's does."""
    play, base = _play_fn(), recs.ctypes.data
    lib, tmp = go.golib(), (ctypes.c_uint8 * 81)()
    for r, mv in zip(np.asarray(rows).tolist(), np.asarray(moves).tolist()):
        if play(base + POS_BYTES * r, mv):
            raise RuntimeError(describe(r, mv))
        if liberties:
            lib.bk_pos_liberties(pos_ptr(recs[r]), tmp)


def area_score_host(recs, komi):
    """bk_pos_area_score of every record, float64 [n]."""
    lib = go.golib()
    return np.array([lib.bk_pos_area_score(pos_ptr(recs[i]), komi) for i in range(len(recs))], np.float64)


def playable_host(recs):
    """bool [n,81]: bk_pos_is_legal(p, s) and bk_pos_possible_eye(p, s) != the colour to move (black on an even turn)."""
    lib = go.golib()
    out = np.zeros((len(recs), 81), bool)
    buf = (ctypes.c_uint8 * 81)()
    for i in range(len(recs)):
        p = pos_ptr(recs[i])
        lib.bk_pos_legal_moves(p, buf)
        mover = 2 if p.contents.turn & 1 else 1
        for s in range(81):
            if buf[s] and lib.bk_pos_possible_eye(p, s) != mover:
                out[i, s] = True
    return out


FEATURE_THREADS = 8        # bk_features_batch_u8 calls in flight per ply (ctypes releases the GIL during each)
FEATURE_CHUNK = 512        # positions per call
_POOL = None


def features_batch(recs, out_ptr):
    """bk_features_batch_u8 over the contiguous bk_pos records recs [n, 192] into out_ptr ([n,27,9,9] uint8), split
    into chunks encoded on FEATURE_THREADS threads: the records are independent, and so are the calls."""
    global _POOL
    lib, n, base = go.golib(), len(recs), recs.ctypes.data
    if n <= FEATURE_CHUNK:
        lib.bk_features_batch_u8(base, n, POS_BYTES, out_ptr, 0)
        return
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(FEATURE_THREADS, thread_name_prefix="bk-features")
    jobs = [_POOL.submit(lib.bk_features_batch_u8, base + POS_BYTES * s, min(FEATURE_CHUNK, n - s), POS_BYTES,
                         out_ptr + PLANE_BYTES * s, 0) for s in range(0, n, FEATURE_CHUNK)]
    for j in jobs:
        j.result()


def initial_positions(n):
    """n empty-board bk_pos records, uint8 [n, 192]."""
    one = np.frombuffer(bytes(go.Game()._pos), np.uint8)
    return np.tile(one, (n, 1))


# ---- the device side ---------------------------------------------------------------------------------------------------------
def engine_logits(pairs):
    """The logits of the rows of every (engine, planes slice) of pairs, in that order, as one tensor: one
    LeafEngine.eval_device per engine.max_batch rows of a slice, none for an empty slice, and no cat for a single part."""
    parts = [eng.eval_device(x[s:s + eng.max_batch], logits=True, probs=False, value=False)["logits"]
             for eng, x in pairs for s in range(0, len(x), eng.max_batch)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def phase_clock(dev, timing):
    """-> lap(name, t0): add the seconds since t0 to timing[name] after a synchronisation of dev and return the time
    now; with timing None it does neither and returns t0."""
    def lap(name, t0):
        if timing is None:
            return t0
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        timing[name] = timing.get(name, 0.0) + (t1 - t0)
        return t1
    return lap


def records_to_device(pos, dev, clone=True):
    """pos (uint8 [G,192], numpy or a tensor) contiguous on dev; clone: a copy the caller may play on in place."""
    pos = (pos.to(dev) if isinstance(pos, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pos)).to(dev))
    return pos.contiguous().clone() if clone else pos.contiguous()


def counters_to_device(counters, G, dev, clone=True):
    """counters (numpy or a tensor) as a contiguous int32 [G,4] tensor on dev; ValueError when they are not that."""
    ctr = (counters.to(dev) if isinstance(counters, torch.Tensor) else
           torch.from_numpy(np.ascontiguousarray(counters, np.int32)).to(dev)).contiguous()
    if tuple(ctr.shape) != (G, 4) or ctr.dtype != torch.int32:
        raise ValueError(f"counters must be int32 [{G}, 4]")
    return ctr.clone() if clone else ctr


def counters_to_host(counters, G):
    """counters (numpy or a tensor) as a fresh int32 [G,4] numpy array; ValueError when they are not that shape."""
    ctr = np.array(counters.cpu().numpy() if hasattr(counters, "cpu") else counters, np.int32)
    if ctr.shape != (G, 4):
        raise ValueError(f"counters must be int32 [{G}, 4]")
    return ctr


def check_status(status, describe):
    """status int32 [n] of the device rules, a tensor or numpy: RuntimeError(describe(row, status)) for the first row
    whose move the rules refused."""
    if bool(status.any()):
        s = int(status.nonzero()[0][0])
        raise RuntimeError(describe(s, int(status[s])))


def check_rules(rules):
    if rules not in ("device", "host"):
        raise ValueError(f"rules must be 'device' or 'host', got {rules!r}")

"""ctypes binding of libbktrain.so (C ABI: include/bokego_train.h), the training kernels of the trunk.

Every call takes torch tensors on the GPU, checks their shapes, and enqueues on torch's current stream.  The library
allocates nothing: outputs and scratch are torch tensors allocated here.  There is no CPU fallback.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbktrain.so")

BKT_ABI_VERSION = 4
COUT = 128
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
STATUS_NAMES = {0: "BKT_OK", -1: "BKT_ERR_ARG", -2: "BKT_ERR_HIP"}

_P = ctypes.c_void_p
_I, _F, _Z, _U64 = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint64
SYMBOLS = {
    "bkt_abi_version": (_I, []),
    "bkt_conv_pack": (_I, [_P, _I, _I, _P, _P]),
    "bkt_conv_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "bkt_conv_pack_dgrad": (_I, [_P, _P, _P]),
    "bkt_conv_dgrad": (_I, [_P, _P, _P, _I, _P]),
    "bkt_conv_wgrad_workspace": (_Z, [_I, _I, _I]),
    "bkt_conv_wgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "bkt_conv_packed_elems_bf16": (_Z, [_I, _I]),
    "bkt_conv_pack_bf16": (_I, [_P, _I, _I, _P, _P]),
    "bkt_conv_forward_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "bkt_conv_pack_dgrad_bf16": (_I, [_P, _P, _P]),
    "bkt_conv_dgrad_bf16": (_I, [_P, _P, _P, _I, _P]),
    "bkt_conv_wgrad_workspace_bf16": (_Z, [_I, _I, _I]),
    "bkt_conv_wgrad_bf16": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P]),
    "bkt_bn_workspace": (_Z, [_I, _I]),
    "bkt_bn_relu_train": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _Z, _I, _I, _P]),
    "bkt_bn_relu_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _I, _P]),
    "bkt_bn_relu_eval": (_I, [_P, _P, _P, _P, _P, _F, _P, _I, _I, _P]),
    "bkt_bn_relu_eval_backward": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _Z, _I, _I, _P]),
    "bkt_sample_moves": (_I, [_P, _P, _I, _U64, _P, _P, _P, _P]),
    "bkt_sample_moves_masked": (_I, [_P, _P, _Z, _I, _U64, _P, _P, _P, _P]),
    "bkt_play_moves": (_I, [_P, _P, _I, _P, _P, _P]),
    "bkt_playout_step": (_I, [_P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_area_score": (_I, [_P, _I, _F, _P, _P, _P]),
    "bkt_random_playouts": (_I, [_P, _I, _U64, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_pattern_codes": (_I, [_P, _I, _P, _P]),
    "bkt_pattern_playouts": (_I, [_P, _I, _U64, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_tactical_codes": (_I, [_P, _I, _P, _P]),
    "bkt_tactical_playouts": (_I, [_P, _I, _U64, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_amaf_counts": (_I, [_P, _I, _P, _I, _I, _P, _P, _P]),
    "bkt_amaf_counts_sides": (_I, [_P, _I, _P, _I, _I, _P, _P, _P]),
    "bkt_owner_counts": (_I, [_P, _I, _I, _F, _P, _P, _P, _P, _P, _P]),
    "bkt_move_weights": (_I, [_P, _I, _P, _P, _P, _P]),
    "bkt_reply_playouts": (_I, [_P, _I, _U64, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_reply_scratch_bytes": (_Z, [_I]),
    "bkt_reply_update": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "bkt_reply_playouts_tables": (_I, [_P, _I, _U64, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_reply_update_tables": (_I, [_P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _P]),
    "bkt_reply2_playouts": (_I, [_P, _I, _U64, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_reply2_scratch_bytes": (_Z, []),
    "bkt_reply2_update": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "bkt_reply2_playouts_tables": (_I, [_P, _I, _U64, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_reply2_tables_scratch_bytes": (_Z, [_I]),
    "bkt_reply2_update_tables": (_I, [_P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _P]),
    "bkt_mm_sums": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "bkt_balance_sums": (_I, [_P, _I, _U64, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_move_value_playouts": (_I, [_P, _I, _U64, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_move_value_scratch_bytes": (_Z, [_I]),
    "bkt_move_value_update": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P]),
    "bkt_move_value_playouts_tables": (_I, [_P, _I, _U64, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_move_value_tables_scratch_bytes": (_Z, [_I, _I]),
    "bkt_move_value_update_tables": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "bkt_move_context_playouts": (_I, [_P, _I, _U64, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "bkt_move_context_scratch_bytes": (_Z, [_I]),
    "bkt_move_context_update": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P]),
}
MAX_BATCH = 65536          # BKT_MAX_BATCH
PRECISIONS = ("fp32", "bf16")
POS_BYTES = 192            # sizeof(bk_pos)
MOVE_NONE = -2             # BKT_MOVE_NONE: bkt_playout_step leaves the row alone
MAX_PLAYOUT_PLIES = 1024   # BKT_MAX_PLAYOUT_PLIES
PATTERN_ENTRIES = 131072   # BKT_PATTERN_ENTRIES
TACTIC_ENTRIES = 64        # BKT_TACTIC_ENTRIES
MAX_SAMPLE_ROWS = 1 << 24  # BKT_MAX_SAMPLE_ROWS
REPLY_NONE = 255           # BKT_REPLY_NONE: a reply table's entry for "no reply"
MM_MAX_ROWS = 16384        # BKT_MM_MAX_ROWS
MM_G_MIN, MM_G_MAX = 1 << 8, 1 << 24   # BKT_MM_G_MIN, BKT_MM_G_MAX: the domain of a fixed-point strength, gamma = g / 65536
BALANCE_Q = 24             # BKT_BALANCE_Q: a share of the draw is booked in units of 2^-24
BALANCE_MAX_ROWS = 16384   # BKT_BALANCE_MAX_ROWS
BALANCE_MAX_COEF = 4096    # BKT_BALANCE_MAX_COEF
MOVE_VALUE_MAX_K = 65536   # BKT_MOVE_VALUE_MAX_K
MOVE_VALUE_MAX_LIMIT = 1 << 30   # BKT_MOVE_VALUE_MAX_LIMIT

_lib = None


def load(path=None):
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `make -C bokego_amd/csrc all`")
    lib = ctypes.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.bkt_abi_version() != BKT_ABI_VERSION:
        raise OSError(f"{p}: ABI version {lib.bkt_abi_version()}, expected {BKT_ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {STATUS_NAMES.get(rc, rc)}")


def _dev(t, name, shape=None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the GPU")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _conv_shape(w):
    if w.dim() != 4 or w.shape[0] != COUT or w.shape[2] != w.shape[3] or w.shape[2] not in (3, 5):
        raise ValueError(f"conv weight must be [128, Cin, k, k] with k 3 or 5, got {tuple(w.shape)}")
    return int(w.shape[1]), int(w.shape[2])


def _batch(x, c):
    if x.dim() != 4 or tuple(x.shape[1:]) != (c, 9, 9):
        raise ValueError(f"expected [B, {c}, 9, 9], got {tuple(x.shape)}")
    return int(x.shape[0])


def _precision(precision):
    """True for "bf16", False for "fp32": the mixed-precision kernels (bf16 GEMM operands rounded once to nearest even,
    fp32 accumulation, fp32 tensors; include/bokego_train.h) or the fp32 ones."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    return precision == "bf16"


def _packed_bf16(cin, k, device):
    n = load().bkt_conv_packed_elems_bf16(cin, k)
    if n == 0:
        raise ValueError(f"unsupported convolution: Cin={cin} k={k}")
    return torch.empty((n,), dtype=torch.int16, device=device)  # bf16 bit patterns in a layout private to the library


def conv_pack(w, precision="fp32"):
    """[128, Cin, k, k] -> the forward operand: [Cin*k*k, 128] fp32, or with precision="bf16" the library's packed bf16
    operand (int16 bit patterns, flat)."""
    bf16 = _precision(precision)
    cin, k = _conv_shape(w)
    if bf16:
        wt = _packed_bf16(cin, k, w.device)
        _check(load().bkt_conv_pack_bf16(_dev(w, "w"), cin, k, _dev(wt, "wt", dtype=torch.int16), _stream(w)),
               "bkt_conv_pack_bf16")
        return wt
    wt = torch.empty((cin * k * k, COUT), dtype=torch.float32, device=w.device)
    _check(load().bkt_conv_pack(_dev(w, "w"), cin, k, _dev(wt, "wt"), _stream(w)), "bkt_conv_pack")
    return wt


def conv_forward(x, w, bias=None, wt=None, precision="fp32"):
    """conv2d(x, w, bias, padding=k//2) on the 9x9 board; wt: conv_pack(w, precision) when the caller already has it."""
    bf16 = _precision(precision)
    cin, k = _conv_shape(w)
    B = _batch(x, cin)
    wt = conv_pack(w, precision) if wt is None else wt
    y = torch.empty((B, COUT, 9, 9), dtype=torch.float32, device=x.device)
    bp = None if bias is None else _dev(bias, "bias", (COUT,))
    if bf16:
        n = load().bkt_conv_packed_elems_bf16(cin, k)
        _check(load().bkt_conv_forward_bf16(_dev(x, "x"), _dev(wt, "wt", (n,), torch.int16), bp, _dev(y, "y"), B, cin, k,
                                            _stream(x)), "bkt_conv_forward_bf16")
        return y
    _check(load().bkt_conv_forward(_dev(x, "x"), _dev(wt, "wt", (cin * k * k, COUT)), bp, _dev(y, "y"), B, cin, k,
                                   _stream(x)), "bkt_conv_forward")
    return y


def conv_dgrad(dy, w, precision="fp32"):
    """dL/dx of the 3x3 128->128 convolution with weights w, from dy = dL/dy."""
    bf16 = _precision(precision)
    cin, k = _conv_shape(w)
    if (cin, k) != (COUT, 3):
        raise ValueError("the input gradient is built for the 3x3 128->128 convolution only")
    B = _batch(dy, COUT)
    lib, s = load(), _stream(dy)
    dx = torch.empty_like(dy)
    if bf16:
        wd = _packed_bf16(COUT, 3, dy.device)
        _check(lib.bkt_conv_pack_dgrad_bf16(_dev(w, "w"), _dev(wd, "wt_dgrad", dtype=torch.int16), s),
               "bkt_conv_pack_dgrad_bf16")
        _check(lib.bkt_conv_dgrad_bf16(_dev(dy, "dy"), _dev(wd, "wt_dgrad", dtype=torch.int16), _dev(dx, "dx"), B, s),
               "bkt_conv_dgrad_bf16")
        return dx
    wd = torch.empty((COUT * 9, COUT), dtype=torch.float32, device=dy.device)
    _check(lib.bkt_conv_pack_dgrad(_dev(w, "w"), _dev(wd, "wt_dgrad"), s), "bkt_conv_pack_dgrad")
    _check(lib.bkt_conv_dgrad(_dev(dy, "dy"), _dev(wd, "wt_dgrad"), _dev(dx, "dx"), B, s), "bkt_conv_dgrad")
    return dx


def conv_wgrad(x, dy, w_shape, need_bias=True, precision="fp32"):
    """(dL/dw [128, Cin, k, k], dL/dbias [128] or None) from the layer input x and dy = dL/dy."""
    bf16 = _precision(precision)
    cin, k = int(w_shape[1]), int(w_shape[2])
    B = _batch(x, cin)
    _batch(dy, COUT)
    if dy.shape[0] != B:
        raise ValueError("x and dy have different batches")
    lib = load()
    workspace, wgrad = ((lib.bkt_conv_wgrad_workspace_bf16, lib.bkt_conv_wgrad_bf16) if bf16 else
                        (lib.bkt_conv_wgrad_workspace, lib.bkt_conv_wgrad))
    nbytes = workspace(B, cin, k)
    if nbytes == 0:
        raise ValueError(f"unsupported convolution: B={B} Cin={cin} k={k}")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)  # 8-byte aligned: it holds double partials
    dw = torch.empty((COUT, cin, k, k), dtype=torch.float32, device=x.device)
    db = torch.empty((COUT,), dtype=torch.float32, device=x.device) if need_bias else None
    _check(wgrad(_dev(x, "x"), _dev(dy, "dy"), _dev(dw, "dw"), None if db is None else _dev(db, "db"), B, cin, k,
                 _dev(ws, "workspace", dtype=torch.float64), nbytes, _stream(x)),
           "bkt_conv_wgrad_bf16" if bf16 else "bkt_conv_wgrad")
    return dw, db


def _bn_workspace(B, C, device):
    nbytes = load().bkt_bn_workspace(B, C)
    if nbytes == 0:
        raise ValueError(f"unsupported BatchNorm: B={B} C={C}")
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device), nbytes


def bn_relu_train(x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None,
                  momentum=BN_MOMENTUM, eps=BN_EPS):
    """Train-mode BatchNorm2d + ReLU; updates the running buffers in place.  -> (y, save_mean, save_invstd)"""
    C = int(gamma.shape[0])
    B = _batch(x, C)
    y = torch.empty_like(x)
    sm = torch.empty((C,), dtype=torch.float32, device=x.device)
    si = torch.empty_like(sm)
    rm = None if running_mean is None else _dev(running_mean, "running_mean", (C,))
    rv = None if running_var is None else _dev(running_var, "running_var", (C,))
    nbt = None if num_batches_tracked is None else _dev(num_batches_tracked, "num_batches_tracked", (), torch.int64)
    ws, nbytes = _bn_workspace(B, C, x.device)
    _check(load().bkt_bn_relu_train(_dev(x, "x"), _dev(gamma, "gamma", (C,)), _dev(beta, "beta", (C,)), rm, rv, nbt,
                                    float(momentum), float(eps), _dev(y, "y"), _dev(sm, "mean"), _dev(si, "invstd"),
                                    _dev(ws, "workspace", dtype=torch.float64), nbytes, B, C, _stream(x)),
           "bkt_bn_relu_train")
    return y, sm, si


def bn_relu_backward(dy, y, x, gamma, save_mean, save_invstd):
    """-> (dx, dgamma, dbeta) of bn_relu_train."""
    C = int(gamma.shape[0])
    B = _batch(x, C)
    dx = torch.empty_like(x)
    dg = torch.empty((C,), dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    ws, nbytes = _bn_workspace(B, C, x.device)
    _check(load().bkt_bn_relu_backward(_dev(dy, "dy", x.shape), _dev(y, "y", x.shape), _dev(x, "x"),
                                       _dev(gamma, "gamma", (C,)), _dev(save_mean, "mean", (C,)),
                                       _dev(save_invstd, "invstd", (C,)), _dev(dx, "dx"), _dev(dg, "dgamma"),
                                       _dev(db, "dbeta"), _dev(ws, "workspace", dtype=torch.float64), nbytes, B, C,
                                       _stream(x)), "bkt_bn_relu_backward")
    return dx, dg, db


def bn_relu_eval(x, gamma, beta, running_mean, running_var, eps=BN_EPS):
    C = int(gamma.shape[0])
    B = _batch(x, C)
    y = torch.empty_like(x)
    _check(load().bkt_bn_relu_eval(_dev(x, "x"), _dev(gamma, "gamma", (C,)), _dev(beta, "beta", (C,)),
                                   _dev(running_mean, "running_mean", (C,)), _dev(running_var, "running_var", (C,)),
                                   float(eps), _dev(y, "y"), B, C, _stream(x)), "bkt_bn_relu_eval")
    return y


def bn_relu_eval_backward(dy, y, x, gamma, running_mean, running_var, eps=BN_EPS):
    """-> (dx, dgamma, dbeta) of bn_relu_eval: the frozen-statistics gradient (no term through the batch statistics)."""
    C = int(gamma.shape[0])
    B = _batch(x, C)
    dx = torch.empty_like(x)
    dg = torch.empty((C,), dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    ws, nbytes = _bn_workspace(B, C, x.device)
    _check(load().bkt_bn_relu_eval_backward(_dev(dy, "dy", x.shape), _dev(y, "y", x.shape), _dev(x, "x"),
                                            _dev(gamma, "gamma", (C,)), _dev(running_mean, "running_mean", (C,)),
                                            _dev(running_var, "running_var", (C,)), float(eps), _dev(dx, "dx"),
                                            _dev(dg, "dgamma"), _dev(db, "dbeta"),
                                            _dev(ws, "workspace", dtype=torch.float64), nbytes, B, C, _stream(x)),
           "bkt_bn_relu_eval_backward")
    return dx, dg, db


def seed_u64(seed):
    """A seed as the unsigned 64-bit integer the kernels take (the Philox key)."""
    return int(seed) & (2 ** 64 - 1)


def _sample(name, logits, mask_args, seed, counters):
    """sample_moves / sample_moves_masked: mask_args(B) checks the second tensor and gives its arguments of the C call."""
    if logits.dim() != 2 or logits.shape[1] != 81:
        raise ValueError(f"logits must be [B, 81], got {tuple(logits.shape)}")
    B = int(logits.shape[0])
    moves = torch.empty((B,), dtype=torch.int32, device=logits.device)
    logp = torch.empty((B,), dtype=torch.float32, device=logits.device)
    if B == 0:
        return moves, logp
    _check(getattr(load(), name)(_dev(logits, "logits"), *mask_args(B), B, seed_u64(seed),
                                 _dev(counters, "counters", (B, 4), torch.int32),
                                 _dev(moves, "moves", dtype=torch.int32), _dev(logp, "logp"), _stream(logits)), name)
    return moves, logp


def sample_moves(logits, planes, seed, counters):
    """One move per row: logits [B,81] f32, planes uint8 [B,27,9,9] (plane 5: legal points), counters int32 [B,4]
    (the Philox counter words, read as uint32) -> (moves int32 [B], -1 where no point is legal; logp f32 [B], NaN on a
    row whose logits are not finite: bokego_train.h, "Degenerate rows")."""
    return _sample("bkt_sample_moves", logits, lambda B: (_dev(planes, "planes", (B, 27, 9, 9), torch.uint8),), seed,
                   counters)


def sample_moves_masked(logits, mask, seed, counters):
    """sample_moves with the acceptable points given as mask uint8 [B,81] (non-zero: may be played) instead of the legal
    plane: the same kernel, the same draw; -1 where a row's mask is empty."""
    return _sample("bkt_sample_moves_masked", logits, lambda B: (_dev(mask, "mask", (B, 81), torch.uint8), 81), seed,
                   counters)


def _pos_batch(pos, ranged=True):
    """B of the records pos [B,192]; ranged: ValueError unless 1 <= B <= MAX_BATCH (else the C side refuses it)."""
    if pos.dim() != 2 or pos.shape[1] != POS_BYTES:
        raise ValueError(f"pos must be [B, {POS_BYTES}], got {tuple(pos.shape)}")
    B = int(pos.shape[0])
    if ranged and not 1 <= B <= MAX_BATCH:
        raise ValueError(f"batch must be 1..{MAX_BATCH}, got {B}")
    return B


def play_moves(pos, moves, planes=None):
    """The Go rules on the device, in place: pos uint8 [B,192] (bk_pos records), moves int32 [B] (< 0: leave the row
    alone) -> status int32 [B] (0 or BK_ILLEGAL_*; an illegal row is untouched).  planes: None, or uint8 [B,27,9,9]
    that receives the features of every record as it stands afterwards (bk_features_batch_u8's)."""
    B = _pos_batch(pos)
    status = torch.empty((B,), dtype=torch.int32, device=pos.device)
    pp = None if planes is None else _dev(planes, "planes", (B, 27, 9, 9), torch.uint8)
    _check(load().bkt_play_moves(_dev(pos, "pos", dtype=torch.uint8), _dev(moves, "moves", (B,), torch.int32), B,
                                 _dev(status, "status", dtype=torch.int32), pp, _stream(pos)), "bkt_play_moves")
    return status


def playout_step(pos, moves, over=None, planes=None, playable=None):
    """One ply of a playout to the end of the game, in place: play_moves that also passes (moves == -1: the second pass
    in a row sets over), leaves rows alone whose move is <= MOVE_NONE or whose over flag is set, and writes playable uint8
    [B,81]: the points the side to move may play in a playout (legal, and not its own one-point eye).  over: None or
    uint8 [B]; planes: None or uint8 [B,27,9,9]; playable: None or uint8 [B,81].  -> status int32 [B]."""
    B = _pos_batch(pos)
    status = torch.empty((B,), dtype=torch.int32, device=pos.device)
    _check(load().bkt_playout_step(_dev(pos, "pos", dtype=torch.uint8), _dev(moves, "moves", (B,), torch.int32), B,
                                   None if over is None else _dev(over, "over", (B,), torch.uint8),
                                   _dev(status, "status", dtype=torch.int32),
                                   None if planes is None else _dev(planes, "planes", (B, 27, 9, 9), torch.uint8),
                                   None if playable is None else _dev(playable, "playable", (B, 81), torch.uint8),
                                   _stream(pos)), "bkt_playout_step")
    return status


def area_score(pos, komi=5.5, owner=False):
    """bk_pos_area_score of every record, on the device: pos uint8 [B,192] (read only) -> score f32 [B], the host's float
    bit for bit; owner=True: (score, owner int8 [B,81]: +1 black stone or black-only empty region, -1 white, 0 neither)."""
    B = _pos_batch(pos, ranged=False)
    score = torch.empty((B,), dtype=torch.float32, device=pos.device)
    own = torch.empty((B, 81), dtype=torch.int8, device=pos.device) if owner else None
    _check(load().bkt_area_score(_dev(pos, "pos", dtype=torch.uint8), B, float(komi), _dev(score, "score"),
                                 None if own is None else _dev(own, "owner", dtype=torch.int8), _stream(pos)),
           "bkt_area_score")
    return (score, own) if owner else score


def _playouts(name, pos, seed, counters, table, max_plies, over, history):
    """bkt_random_playouts, or bkt_pattern_playouts / bkt_tactical_playouts with their table arguments after the counters."""
    B, max_plies = _pos_batch(pos), int(max_plies)
    if not 1 <= max_plies <= MAX_PLAYOUT_PLIES:
        raise ValueError(f"max_plies must be 1..{MAX_PLAYOUT_PLIES}, got {max_plies}")
    if over is None:
        over = torch.zeros((B,), dtype=torch.uint8, device=pos.device)
    plies = torch.empty((B,), dtype=torch.int32, device=pos.device)
    status = torch.empty((B,), dtype=torch.int32, device=pos.device)
    moves = torch.empty((B, max_plies), dtype=torch.int16, device=pos.device) if history else None
    _check(getattr(load(), name)(_dev(pos, "pos", dtype=torch.uint8), B, seed_u64(seed),
                                 _dev(counters, "counters", (B, 4), torch.int32), *table, max_plies,
                                 _dev(over, "over", (B,), torch.uint8), _dev(plies, "plies", dtype=torch.int32),
                                 None if moves is None else _dev(moves, "moves", dtype=torch.int16),
                                 _dev(status, "status", dtype=torch.int32), _stream(pos)), name)
    return over, plies, moves, status


def random_playouts(pos, seed, counters, max_plies, over=None, history=True):
    """Whole uniformly random playouts in one launch, in place (bkt_random_playouts): pos uint8 [B,192], counters int32
    [B,4] (the Philox counter words of ply 0; word 1 runs on with the ply), 1 <= max_plies <= MAX_PLAYOUT_PLIES.  over: None
    (no game has ended) or uint8 [B], updated in place; rows whose flag is set are left alone.
    -> (over uint8 [B], plies int32 [B], moves int16 [B,max_plies] or None with history=False, status int32 [B])."""
    return _playouts("bkt_random_playouts", pos, seed, counters, (), max_plies, over, history)


def pattern_playouts(pos, seed, counters, table, max_plies, over=None, history=True):
    """random_playouts with the pattern-weighted draw (bkt_pattern_playouts): table int16 [PATTERN_ENTRIES] on the device of
    pos, the bits of the uint16 weights (torch has no uint16 arithmetic; nothing here computes with them)."""
    if table.device != pos.device:
        raise ValueError("the pattern table must be on the device of pos")
    return _playouts("bkt_pattern_playouts", pos, seed, counters, (_dev(table, "table", (PATTERN_ENTRIES,), torch.int16),),
                     max_plies, over, history)


def pattern_codes(pos):
    """The 3x3 pattern index of every point (bkt_pattern_codes): pos uint8 [B,192] (read only) -> int32 [B,81]."""
    B = _pos_batch(pos)
    codes = torch.empty((B, 81), dtype=torch.int32, device=pos.device)
    _check(load().bkt_pattern_codes(_dev(pos, "pos", dtype=torch.uint8), B, _dev(codes, "codes", dtype=torch.int32),
                                    _stream(pos)), "bkt_pattern_codes")
    return codes


def _weight_tables(pos, table, tactics):
    """(table, tactics) as the C calls take them, None staying NULL: each a tensor on the device of pos."""
    for t in (table, tactics):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device != pos.device):
            raise ValueError("the pattern table and the tactics table must be on the device of pos")
    return (None if table is None else _dev(table, "table", (PATTERN_ENTRIES,), torch.int16),
            None if tactics is None else _dev(tactics, "tactics", (TACTIC_ENTRIES,), torch.int16))


def tactical_playouts(pos, seed, counters, table, tactics, max_plies, over=None, history=True):
    """pattern_playouts whose weights are multiplied by a second table (bkt_tactical_playouts): tactics int16
    [TACTIC_ENTRIES] on the device of pos, the bits of the uint16 entries (256: neutral), indexed by the tactical code;
    table: pattern_playouts' table, or None for no patterns (every pattern weight 256)."""
    return _playouts("bkt_tactical_playouts", pos, seed, counters, _weight_tables(pos, table, tactics), max_plies, over, history)


def tactical_codes(pos):
    """The tactical code of every point (bkt_tactical_codes): pos uint8 [B,192] (read only) -> int32 [B,81]."""
    B = _pos_batch(pos)
    codes = torch.empty((B, 81), dtype=torch.int32, device=pos.device)
    _check(load().bkt_tactical_codes(_dev(pos, "pos", dtype=torch.uint8), B, _dev(codes, "codes", dtype=torch.int32),
                                     _stream(pos)), "bkt_tactical_codes")
    return codes


def _sample_rows(records, playouts):
    """records and playouts as ints, in the range of the reductions over records * playouts rows."""
    records, playouts = int(records), int(playouts)
    if records < 1 or playouts < 1 or records * playouts > MAX_SAMPLE_ROWS:
        raise ValueError(f"records and playouts must be at least 1 and records * playouts at most {MAX_SAMPLE_ROWS}, "
                         f"got {records} x {playouts}")
    return records, playouts


def _amaf_args(moves, won, records, playouts):
    """The checks amaf_counts, amaf_counts_sides and reply_update share -> (records, playouts, max_plies)."""
    records, playouts = _sample_rows(records, playouts)
    if not isinstance(moves, torch.Tensor) or moves.dim() != 2 or moves.shape[0] != records * playouts:
        raise ValueError(f"moves must be [{records * playouts}, max_plies]")
    max_plies = int(moves.shape[1])
    if not 1 <= max_plies <= MAX_PLAYOUT_PLIES:
        raise ValueError(f"max_plies must be 1..{MAX_PLAYOUT_PLIES}, got {max_plies}")
    if isinstance(won, torch.Tensor) and won.device != moves.device:
        raise ValueError("won must be on the device of moves")
    return records, playouts, max_plies


def amaf_counts(moves, won, records, playouts):
    """The all-moves-as-first counts of whole playouts (bkt_amaf_counts): moves int16 [records * playouts, max_plies], the
    history random_playouts / pattern_playouts / tactical_playouts write, rows r * playouts .. of record r; won uint8
    [records * playouts], non-zero where the side to move at the record won the row's playout.
    -> (played int32 [records, 81], won_at int32 [records, 81]): the rows in which the side to move was the first to play
    the point, and those of them it won."""
    records, playouts, max_plies = _amaf_args(moves, won, records, playouts)
    played = torch.empty((records, 81), dtype=torch.int32, device=moves.device)
    won_at = torch.empty((records, 81), dtype=torch.int32, device=moves.device)
    _check(load().bkt_amaf_counts(_dev(moves, "moves", dtype=torch.int16), max_plies,
                                  _dev(won, "won", (records * playouts,), torch.uint8), records, playouts,
                                  _dev(played, "played", dtype=torch.int32), _dev(won_at, "won_at", dtype=torch.int32),
                                  _stream(moves)), "bkt_amaf_counts")
    return played, won_at


def amaf_counts_sides(moves, won, records, playouts):
    """amaf_counts for both sides of every history (bkt_amaf_counts_sides): the same moves and won
    -> (played int32 [records, 2, 81], won_at int32 [records, 2, 81]): side 0 is the side to move at the record -- its rows
    are amaf_counts' output -- and side 1 its opponent: the rows in which that side was the first to play the point, and
    those of them it won (the opponent wins a row whose won is 0)."""
    records, playouts, max_plies = _amaf_args(moves, won, records, playouts)
    played = torch.empty((records, 2, 81), dtype=torch.int32, device=moves.device)
    won_at = torch.empty((records, 2, 81), dtype=torch.int32, device=moves.device)
    _check(load().bkt_amaf_counts_sides(_dev(moves, "moves", dtype=torch.int16), max_plies,
                                        _dev(won, "won", (records * playouts,), torch.uint8), records, playouts,
                                        _dev(played, "played", dtype=torch.int32), _dev(won_at, "won_at", dtype=torch.int32),
                                        _stream(moves)), "bkt_amaf_counts_sides")
    return played, won_at


def owner_counts(pos, records, playouts, komi=5.5):
    """The ownership, agreement and score-margin counts of whole playouts (bkt_owner_counts; include/bokego_train.h has the
    definition): pos uint8 [records * playouts, 192], the final records (read only), rows r * playouts .. of record r
    -> (black int32 [records, 81], white int32 [records, 81], agree int32 [records, 81], hist int32 [records, 163],
    black_wins int32 [records]): the playouts in which the point ended up black's, white's and the winner's, the playouts
    by their margin B - W + 81 before komi, and those black won (bkt_area_score's score > 0)."""
    records, playouts = _sample_rows(records, playouts)
    if not isinstance(pos, torch.Tensor) or pos.dim() != 2 or tuple(pos.shape) != (records * playouts, POS_BYTES):
        raise ValueError(f"pos must be [{records * playouts}, {POS_BYTES}]")
    komi = float(komi)
    if komi - komi != 0.0:
        raise ValueError("komi must be finite")
    black, white, agree = (torch.empty((records, 81), dtype=torch.int32, device=pos.device) for _ in range(3))
    hist = torch.empty((records, 163), dtype=torch.int32, device=pos.device)
    black_wins = torch.empty((records,), dtype=torch.int32, device=pos.device)
    _check(load().bkt_owner_counts(_dev(pos, "pos", dtype=torch.uint8), records, playouts, komi,
                                   _dev(black, "black", dtype=torch.int32), _dev(white, "white", dtype=torch.int32),
                                   _dev(agree, "agree", dtype=torch.int32), _dev(hist, "hist", dtype=torch.int32),
                                   _dev(black_wins, "black_wins", dtype=torch.int32), _stream(pos)), "bkt_owner_counts")
    return black, white, agree, hist, black_wins


def move_weights(pos, table=None, tactics=None):
    """The move weights of every record in one launch (bkt_move_weights; include/bokego_train.h has the definition): pos
    uint8 [B,192] (read only); table: None or pattern_playouts' table; tactics: None or tactical_playouts' table
    -> int32 [B,81]: the weight tactical_playouts' draw gives the point at the first ply from the record (below 2^24), 0
    where the point is not playable."""
    B = _pos_batch(pos)
    tables = _weight_tables(pos, table, tactics)
    weights = torch.empty((B, 81), dtype=torch.int32, device=pos.device)
    _check(load().bkt_move_weights(_dev(pos, "pos", dtype=torch.uint8), B, *tables,
                                   _dev(weights, "weights", dtype=torch.int32), _stream(pos)), "bkt_move_weights")
    return weights


def reply_playouts(pos, seed, counters, table, tactics, replies, max_plies, over=None, history=True, slots=None):
    """tactical_playouts whose draw asks a last-good-reply table first (bkt_reply_playouts; include/bokego_train.h has the
    rule): replies uint8 [2,81] on the device of pos, read only; table and tactics: tactical_playouts' tables, each of which
    may be None here (neither: the uniform draw).  With slots, many tables in the same launch (bkt_reply_playouts_tables):
    replies uint8 [tables,2,81] and slots int32 [B] on the device of pos, both read only; row i asks table slots[i], and a
    slot outside 0..tables-1 plays as an empty table."""
    weights = _weight_tables(pos, table, tactics)
    suffix, tables = _reply_tables(replies, slots, _pos_batch(pos), pos.device, "pos")
    return _playouts("bkt_reply_playouts" + suffix, pos, seed, counters, (*weights, *tables), max_plies, over, history)


def reply_update(pos, moves, won, records, playouts, replies, scratch=None, slots=None):
    """Fold a batch of playouts into a last-good-reply table, in place (bkt_reply_update; include/bokego_train.h has the
    rule): pos uint8 [records,192], the starting records (read only); moves and won as amaf_counts_sides takes them; replies
    uint8 [2,81].  scratch: None (allocated here) or a uint8 tensor of at least bkt_reply_scratch_bytes(records) bytes.
    With slots, many tables (bkt_reply_update_tables): replies uint8 [tables,2,81]; slots int32 [records], the table of every
    record -- table t is folded with the records whose slot is t, in ascending order; a slot outside 0..tables-1 updates
    nothing.  Two launches on the current stream either way; nothing waits.  -> replies."""
    records, playouts, max_plies = _amaf_args(moves, won, records, playouts)
    if not isinstance(pos, torch.Tensor) or tuple(pos.shape) != (records, POS_BYTES) or pos.device != moves.device:
        raise ValueError(f"pos must be [{records}, {POS_BYTES}] on the device of moves")
    suffix, tables = _reply_tables(replies, slots, records, moves.device, "moves")
    name = "bkt_reply_update" + suffix
    need = load().bkt_reply_scratch_bytes(records)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=moves.device)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != moves.device or scratch.dim() != 1 or scratch.numel() < need:
        raise ValueError(f"scratch must be uint8 [>= {need}] on the device of moves")
    _check(getattr(load(), name)(_dev(pos, "pos", dtype=torch.uint8), _dev(moves, "moves", dtype=torch.int16), max_plies,
                                 _dev(won, "won", (records * playouts,), torch.uint8), records, playouts, *tables,
                                 _dev(scratch, "scratch", dtype=torch.uint8), _stream(moves)), name)
    return replies


def _reply_tables(replies, slots, n, dev, what):
    """replies, and slots for n rows, as the C calls take them -> ("", (replies,)) for the single table of slots=None, else
    ("_tables", (replies, tables, slots)): the suffix of the symbol and its table arguments."""
    if not isinstance(replies, torch.Tensor) or replies.device != dev or (slots is not None and replies.dim() != 3):
        raise ValueError(f"replies must be uint8 [2, 81], or with slots [tables, 2, 81], on the device of {what}")
    if slots is None:
        return "", (_dev(replies, "replies", (2, 81), torch.uint8),)
    tables = int(replies.shape[0])
    if not 1 <= tables <= MAX_BATCH:
        raise ValueError(f"the number of reply tables must be 1..{MAX_BATCH}, got {tables}")
    if not isinstance(slots, torch.Tensor) or slots.device != dev:
        raise ValueError(f"slots must be int32 [{n}] on the device of {what}")
    return "_tables", (_dev(replies, "replies", (tables, 2, 81), torch.uint8), tables, _dev(slots, "slots", (n,), torch.int32))


def reply_playouts_tables(pos, seed, counters, table, tactics, replies, slots, max_plies, over=None, history=True):
    """reply_playouts with slots, by position."""
    return reply_playouts(pos, seed, counters, table, tactics, replies, max_plies, over, history, slots)


def reply_update_tables(pos, moves, won, records, playouts, replies, slots, scratch=None):
    """reply_update with slots, by position."""
    return reply_update(pos, moves, won, records, playouts, replies, scratch, slots)


MAX_REPLY2_TABLES = 4096   # BKT_MAX_REPLY2_TABLES
_reply2_scratch = {}       # (device, stream, bytes) -> the scratch of reply2_update with slots


def _reply2_table(replies2, dev, what):
    if not isinstance(replies2, torch.Tensor) or replies2.device != dev:
        raise ValueError(f"replies2 must be uint8 [2, 82, 81] on the device of {what}")
    return _dev(replies2, "replies2", (2, 82, 81), torch.uint8)


def _reply2_tables(replies2, slots, n, dev, what):
    """_reply_tables for pair tables -> ("", (replies2,)) for the single table of slots=None, else ("_tables", (replies2,
    tables, slots))."""
    if slots is None:
        return "", (_reply2_table(replies2, dev, what),)
    if not isinstance(replies2, torch.Tensor) or replies2.device != dev or replies2.dim() != 4:
        raise ValueError(f"replies2 must with slots be uint8 [tables, 2, 82, 81] on the device of {what}")
    tables = int(replies2.shape[0])
    if not 1 <= tables <= MAX_REPLY2_TABLES:
        raise ValueError(f"the number of pair reply tables must be 1..{MAX_REPLY2_TABLES}, got {tables}")
    if not isinstance(slots, torch.Tensor) or slots.device != dev:
        raise ValueError(f"slots must be int32 [{n}] on the device of {what}")
    return "_tables", (_dev(replies2, "replies2", (tables, 2, 82, 81), torch.uint8), tables,
                       _dev(slots, "slots", (n,), torch.int32))


def reply2_playouts(pos, seed, counters, table, tactics, replies2, max_plies, over=None, history=True, slots=None):
    """reply_playouts whose table is keyed by the last two moves (bkt_reply2_playouts; include/bokego_train.h has the rule):
    replies2 uint8 [2,82,81] on the device of pos, read only, plane 81 being reply_playouts' table; one table for all rows.
    With slots, many tables in the same launch (bkt_reply2_playouts_tables): replies2 uint8 [tables,2,82,81] and slots int32
    [B] on the device of pos, both read only; row i asks table slots[i], and a slot outside 0..tables-1 plays as an empty
    table."""
    weights = _weight_tables(pos, table, tactics)
    suffix, tables = _reply2_tables(replies2, slots, _pos_batch(pos), pos.device, "pos")
    return _playouts("bkt_reply2_playouts" + suffix, pos, seed, counters, (*weights, *tables), max_plies, over, history)


def reply2_update(pos, moves, won, records, playouts, replies2, scratch=None, slots=None):
    """Fold a batch of playouts into a pair reply table, in place (bkt_reply2_update; include/bokego_train.h has the rule):
    reply_update's arguments with replies2 uint8 [2,82,81].  scratch: None (allocated here) or a uint8 tensor of at least
    bkt_reply2_scratch_bytes() bytes, 8-byte aligned.  Four launches on the current stream; nothing waits.
    With slots, many tables (bkt_reply2_update_tables): replies2 uint8 [tables,2,82,81]; slots int32 [records], the table of
    every record -- table t is folded with the records whose slot is t, in ascending order; a slot outside 0..tables-1
    updates nothing.  The scratch is then bkt_reply2_tables_scratch_bytes(tables) bytes, and the one allocated here is
    kept per device, stream and size: the launches that use it are ordered by the stream.  -> replies2."""
    records, playouts, max_plies = _amaf_args(moves, won, records, playouts)
    if not isinstance(pos, torch.Tensor) or tuple(pos.shape) != (records, POS_BYTES) or pos.device != moves.device:
        raise ValueError(f"pos must be [{records}, {POS_BYTES}] on the device of moves")
    suffix, tables = _reply2_tables(replies2, slots, records, moves.device, "moves")
    name = "bkt_reply2_update" + suffix
    need = load().bkt_reply2_scratch_bytes() if slots is None else load().bkt_reply2_tables_scratch_bytes(tables[1])
    if scratch is None and slots is not None:
        key = (moves.device, torch.cuda.current_stream(moves.device).cuda_stream, need)
        if key not in _reply2_scratch:
            _reply2_scratch[key] = torch.empty((need,), dtype=torch.uint8, device=moves.device)
        scratch = _reply2_scratch[key]
    elif scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=moves.device)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != moves.device or scratch.dim() != 1 or scratch.numel() < need:
        raise ValueError(f"scratch must be uint8 [>= {need}] on the device of moves")
    _check(getattr(load(), name)(_dev(pos, "pos", dtype=torch.uint8), _dev(moves, "moves", dtype=torch.int16), max_plies,
                                 _dev(won, "won", (records * playouts,), torch.uint8), records, playouts, *tables,
                                 _dev(scratch, "scratch", dtype=torch.uint8), _stream(moves)), name)
    return replies2


MAX_MOVE_VALUE_TABLES = 4096   # BKT_MAX_MOVE_VALUE_TABLES


def _move_values(values, dev, what):
    if not isinstance(values, torch.Tensor) or values.device != dev:
        raise ValueError(f"values must be int16 [2, 81] (the bits of the uint16 entries) on the device of {what}")
    return _dev(values, "values", (2, 81), torch.int16)


def _move_value_tables(values, slots, n, dev, what):
    """values int16 [tables,2,81] and slots int32 [n] as the *_tables calls take them -> (values, tables, slots)."""
    if not isinstance(values, torch.Tensor) or values.device != dev or values.dim() != 3:
        raise ValueError(f"values must with slots be int16 [tables, 2, 81] (the bits of the uint16 entries) on the device of {what}")
    tables = int(values.shape[0])
    if not 1 <= tables <= MAX_MOVE_VALUE_TABLES:
        raise ValueError(f"the number of move-value tables must be 1..{MAX_MOVE_VALUE_TABLES}, got {tables}")
    if not isinstance(slots, torch.Tensor) or slots.device != dev:
        raise ValueError(f"slots must be int32 [{n}] on the device of {what}")
    return _dev(values, "values", (tables, 2, 81), torch.int16), tables, _dev(slots, "slots", (n,), torch.int32)


def move_value_playouts(pos, seed, counters, table, tactics, values, max_plies, over=None, history=True, replies=None,
                        replies2=None, slots=None):
    """tactical_playouts whose weights are multiplied by a per-(colour, point) factor (bkt_move_value_playouts;
    include/bokego_train.h has the rule): values int16 [2,81] on the device of pos, the bits of the uint16 entries (256:
    neutral), read only; table and tactics: tactical_playouts' tables, each of which may be None.  replies: None or
    reply_playouts' table, uint8 [2,81]; replies2: None or reply2_playouts' table, uint8 [2,82,81]; at most one of the two
    (ValueError): a playable reply overrules the draw as in those calls.
    With slots, many tables in the same launch (bkt_move_value_playouts_tables): values int16 [tables,2,81] and slots int32
    [B] on the device of pos, both read only; row i draws with table slots[i], and a slot outside 0..tables-1 plays as if
    every value were 256.  replies is then uint8 [tables,2,81] and replies2 uint8 [tables,2,82,81], with the same number of
    tables: the same slot names the reply table and the move-value table of a row."""
    weights = _weight_tables(pos, table, tactics)
    if replies is not None and replies2 is not None:
        raise ValueError("at most one of replies and replies2 may be given: a pair table contains the single one")
    if slots is not None:
        B = _pos_batch(pos)
        v, tables, sl = _move_value_tables(values, slots, B, pos.device, "pos")
        r1 = None if replies is None else _reply_tables(replies, slots, B, pos.device, "pos")[1]
        r2 = None if replies2 is None else _reply2_tables(replies2, slots, B, pos.device, "pos")[1]
        for r in (r1, r2):
            if r is not None and r[1] != tables:
                raise ValueError(f"the reply tables and the move-value tables must be equally many, got {r[1]} and {tables}")
        return _playouts("bkt_move_value_playouts_tables", pos, seed, counters,
                         (*weights, v, None if r1 is None else r1[0], None if r2 is None else r2[0], tables, sl), max_plies,
                         over, history)
    v = _move_values(values, pos.device, "pos")
    r1 = None if replies is None else _reply_tables(replies, None, _pos_batch(pos), pos.device, "pos")[1][0]
    r2 = None if replies2 is None else _reply2_table(replies2, pos.device, "pos")
    return _playouts("bkt_move_value_playouts", pos, seed, counters, (*weights, v, r1, r2), max_plies, over, history)


def move_value_update(pos, moves, won, records, playouts, counts, values, lut, k, limit, scratch=None, slots=None):
    """Fold a batch of playouts into a move-value table, in place (bkt_move_value_update; include/bokego_train.h has the
    rule): pos uint8 [records,192], the starting records (read only); moves and won as reply_update takes them; counts int64
    [2,81,2], values int16 [2,81] and lut int16 [65] (the bits of the uint16 entries) on the device of moves; 1 <= k <=
    MOVE_VALUE_MAX_K; limit 0 or 2..MOVE_VALUE_MAX_LIMIT; playouts * max_plies < 2^31.  scratch: None (allocated here) or a
    uint8 tensor of at least bkt_move_value_scratch_bytes(records) bytes.  Two launches on the current stream; nothing
    waits.
    With slots, many tables (bkt_move_value_update_tables): counts int64 [tables,2,81,2] and values int16 [tables,2,81];
    slots int32 [records], the table of every record -- table t is updated with the records whose slot is t, a table that
    no record names keeps every byte, and a slot outside 0..tables-1 updates nothing.  -> (counts, values)."""
    records, playouts, max_plies = _amaf_args(moves, won, records, playouts)
    if not isinstance(pos, torch.Tensor) or tuple(pos.shape) != (records, POS_BYTES) or pos.device != moves.device:
        raise ValueError(f"pos must be [{records}, {POS_BYTES}] on the device of moves")
    k, limit = int(k), int(limit)
    if not 1 <= k <= MOVE_VALUE_MAX_K:
        raise ValueError(f"k must be 1..{MOVE_VALUE_MAX_K}, got {k}")
    if limit != 0 and not 2 <= limit <= MOVE_VALUE_MAX_LIMIT:
        raise ValueError(f"limit must be 0 or 2..{MOVE_VALUE_MAX_LIMIT}, got {limit}")
    if playouts * max_plies >= 2 ** 31:
        raise ValueError("playouts * max_plies must be below 2^31: a record's partial counts are int32")
    for t, name in ((counts, "counts"), (lut, "lut")):
        if not isinstance(t, torch.Tensor) or t.device != moves.device:
            raise ValueError(f"{name} must be on the device of moves")
    if slots is None:
        v, extra, shape, name = _move_values(values, moves.device, "moves"), (), (2, 81, 2), "bkt_move_value_update"
        need = load().bkt_move_value_scratch_bytes(records)
    else:
        v, tables, sl = _move_value_tables(values, slots, records, moves.device, "moves")
        extra, shape, name = (tables, sl), (tables, 2, 81, 2), "bkt_move_value_update_tables"
        need = load().bkt_move_value_tables_scratch_bytes(records, tables)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=moves.device)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != moves.device or scratch.dim() != 1 or scratch.numel() < need:
        raise ValueError(f"scratch must be uint8 [>= {need}] on the device of moves")
    _check(getattr(load(), name)(_dev(pos, "pos", dtype=torch.uint8), _dev(moves, "moves", dtype=torch.int16), max_plies,
                                 _dev(won, "won", (records * playouts,), torch.uint8), records, playouts,
                                 _dev(counts, "counts", shape, torch.int64), v, _dev(lut, "lut", (65,), torch.int16),
                                 k, limit, *extra, _dev(scratch, "scratch", dtype=torch.uint8), _stream(moves)), name)
    return counts, values


MOVE_CONTEXT_MAX_MIN_PLAYS = 1 << 30   # BKT_MOVE_CONTEXT_MAX_MIN_PLAYS


def _move_contexts(values, dev, what):
    if not isinstance(values, torch.Tensor) or values.device != dev:
        raise ValueError(f"values must be int16 [2, 82, 81] (the bits of the uint16 entries) on the device of {what}")
    return _dev(values, "values", (2, 82, 81), torch.int16)


def move_context_scratch_bytes(records):
    """bkt_move_context_scratch_bytes: the bytes of move_context_update's scratch (0 when records < 1)."""
    return int(load().bkt_move_context_scratch_bytes(int(records)))


def move_context_playouts(pos, seed, counters, table, tactics, values, max_plies, over=None, history=True, replies=None,
                          replies2=None):
    """move_value_playouts whose factor is keyed by the previous move as well (bkt_move_context_playouts;
    include/bokego_train.h has the rule): values int16 [2,82,81] on the device of pos, the bits of the uint16 entries (256:
    neutral), read only, plane 81 being move_value_playouts' table; one table for all rows.  table, tactics, replies and
    replies2: as move_value_playouts takes them, at most one of the last two (ValueError)."""
    weights = _weight_tables(pos, table, tactics)
    if replies is not None and replies2 is not None:
        raise ValueError("at most one of replies and replies2 may be given: a pair table contains the single one")
    v = _move_contexts(values, pos.device, "pos")
    r1 = None if replies is None else _reply_tables(replies, None, _pos_batch(pos), pos.device, "pos")[1][0]
    r2 = None if replies2 is None else _reply2_table(replies2, pos.device, "pos")
    return _playouts("bkt_move_context_playouts", pos, seed, counters, (*weights, v, r1, r2), max_plies, over, history)


def move_context_update(pos, moves, won, records, playouts, counts, values, lut, k, limit, min_plays, scratch=None):
    """Fold a batch of playouts into a move-context table, in place (bkt_move_context_update; include/bokego_train.h has the
    rule): move_value_update's arguments with counts int64 [2,82,81,2] and values int16 [2,82,81], and min_plays
    1..MOVE_CONTEXT_MAX_MIN_PLAYS, the plays a context entry needs before it counts.  scratch: None (allocated here) or a
    uint8 tensor of at least bkt_move_context_scratch_bytes(records) bytes, 8-byte aligned.  Three launches on the current
    stream; nothing waits.  -> (counts, values)."""
    records, playouts, max_plies = _amaf_args(moves, won, records, playouts)
    if not isinstance(pos, torch.Tensor) or tuple(pos.shape) != (records, POS_BYTES) or pos.device != moves.device:
        raise ValueError(f"pos must be [{records}, {POS_BYTES}] on the device of moves")
    k, limit, min_plays = int(k), int(limit), int(min_plays)
    if not 1 <= k <= MOVE_VALUE_MAX_K:
        raise ValueError(f"k must be 1..{MOVE_VALUE_MAX_K}, got {k}")
    if limit != 0 and not 2 <= limit <= MOVE_VALUE_MAX_LIMIT:
        raise ValueError(f"limit must be 0 or 2..{MOVE_VALUE_MAX_LIMIT}, got {limit}")
    if not 1 <= min_plays <= MOVE_CONTEXT_MAX_MIN_PLAYS:
        raise ValueError(f"min_plays must be 1..{MOVE_CONTEXT_MAX_MIN_PLAYS}, got {min_plays}")
    if playouts * max_plies >= 2 ** 31:
        raise ValueError("playouts * max_plies must be below 2^31, as for move_value_update")
    for t, name in ((counts, "counts"), (lut, "lut")):
        if not isinstance(t, torch.Tensor) or t.device != moves.device:
            raise ValueError(f"{name} must be on the device of moves")
    v = _move_contexts(values, moves.device, "moves")
    need = load().bkt_move_context_scratch_bytes(records)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=moves.device)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != moves.device or scratch.dim() != 1 or scratch.numel() < need:
        raise ValueError(f"scratch must be uint8 [>= {need}] on the device of moves")
    _check(load().bkt_move_context_update(_dev(pos, "pos", dtype=torch.uint8), _dev(moves, "moves", dtype=torch.int16), max_plies,
                                          _dev(won, "won", (records * playouts,), torch.uint8), records, playouts,
                                          _dev(counts, "counts", (2, 82, 81, 2), torch.int64), v,
                                          _dev(lut, "lut", (65,), torch.int16), k, limit, min_plays,
                                          _dev(scratch, "scratch", dtype=torch.uint8), _stream(moves)),
           "bkt_move_context_update")
    return counts, values


def mm_strengths(g, entries, name, device=None):
    """A strength table as bkt_mm_sums takes it: g, integers [entries] (numpy or a tensor), each MM_G_MIN..MM_G_MAX -- else
    ValueError, before any launch -> int32 [entries] (the bits of the uint32 words), on `device` when one is given."""
    if hasattr(g, "astype") and g.dtype.kind in "iu":
        g = g.astype("int64")                                           # numpy's unsigned types: torch has no arithmetic on them
    t = g if isinstance(g, torch.Tensor) else torch.as_tensor(g)
    if t.dim() != 1 or t.shape[0] != entries or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{name} must be integers [{entries}], got {t.dtype} {tuple(t.shape)}")
    t = t.to(torch.int64)
    if int(t.min()) < MM_G_MIN or int(t.max()) > MM_G_MAX:
        raise ValueError(f"{name}: a strength is {MM_G_MIN}..{MM_G_MAX} (gamma = g / 65536 in [2^-8, 2^8]), got "
                         f"{int(t.min())}..{int(t.max())}")
    t = t.to(torch.int32)
    return t if device is None else t.to(device)


def mm_sums(codes, moves, gp, gt, den_p=None, den_t=None):
    """One MM pass over packed positions (bkt_mm_sums; include/bokego_train.h has the definition): codes int32 [R,81] (the
    bits of the uint32 words) and moves int32 [R] on the device, any R >= 1: one launch per MM_MAX_ROWS rows.  gp, gt: the
    strengths, integers [PATTERN_ENTRIES] and [TACTIC_ENTRIES] on any device; a strength outside MM_G_MIN..MM_G_MAX is a
    ValueError before any launch.  den_p, den_t: None (zeroed here) or int64 [PATTERN_ENTRIES] / [TACTIC_ENTRIES] on the
    device of codes (the bits of the uint64 sums), added to.
    -> (den_p, den_t, total int64 [R], chosen int64 [R], rank int32 [R])."""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.shape[1] != 81 or codes.shape[0] < 1:
        raise ValueError("codes must be int32 [R, 81] with R >= 1")
    R, dev = int(codes.shape[0]), codes.device
    cp, mp = _dev(codes, "codes", dtype=torch.int32), _dev(moves, "moves", (R,), torch.int32)
    if moves.device != dev:
        raise ValueError("moves must be on the device of codes")
    gp, gt = mm_strengths(gp, PATTERN_ENTRIES, "gp", dev), mm_strengths(gt, TACTIC_ENTRIES, "gt", dev)
    den_p = torch.zeros((PATTERN_ENTRIES,), dtype=torch.int64, device=dev) if den_p is None else den_p
    den_t = torch.zeros((TACTIC_ENTRIES,), dtype=torch.int64, device=dev) if den_t is None else den_t
    if den_p.device != dev or den_t.device != dev:
        raise ValueError("den_p and den_t must be on the device of codes")
    dp, dt = _dev(den_p, "den_p", (PATTERN_ENTRIES,), torch.int64), _dev(den_t, "den_t", (TACTIC_ENTRIES,), torch.int64)
    total = torch.empty((R,), dtype=torch.int64, device=dev)
    chosen = torch.empty((R,), dtype=torch.int64, device=dev)
    rank = torch.empty((R,), dtype=torch.int32, device=dev)
    lib, stream = load(), _stream(codes)
    for s in range(0, R, MM_MAX_ROWS):
        n = min(MM_MAX_ROWS, R - s)
        _check(lib.bkt_mm_sums(cp + s * 81 * 4, mp + s * 4, n, _dev(gp, "gp", dtype=torch.int32), _dev(gt, "gt", dtype=torch.int32),
                               dp, dt, total.data_ptr() + s * 8, chosen.data_ptr() + s * 8, rank.data_ptr() + s * 4, stream),
               "bkt_mm_sums")
    return den_p, den_t, total, chosen, rank


def balance_coef(coef, rows, device=None):
    """A coefficient per row as bkt_balance_sums takes them: coef, integers [rows] (numpy or a tensor), each at most
    BALANCE_MAX_COEF in magnitude -- else ValueError, before any launch -> int32 [rows], on `device` when one is given."""
    t = coef if isinstance(coef, torch.Tensor) else torch.as_tensor(coef)
    if t.dim() != 1 or t.shape[0] != rows or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"coef must be integers [{rows}], got {t.dtype} {tuple(t.shape)}")
    t = t.to(torch.int64)
    if rows and (int(t.min()) < -BALANCE_MAX_COEF or int(t.max()) > BALANCE_MAX_COEF):
        raise ValueError(f"coef: a coefficient is -{BALANCE_MAX_COEF}..{BALANCE_MAX_COEF} (the sums of a call then stay below "
                         f"2^61), got {int(t.min())}..{int(t.max())}")
    t = t.to(torch.int32).contiguous()
    return t if device is None else t.to(device)


def balance_sums(pos, seed, counters, table, tactics, coef, max_plies, over=None, history=True, grad_p=None, grad_t=None):
    """The gradient sums of simulation balancing (bkt_balance_sums; include/bokego_train.h has the definition):
    tactical_playouts -- pos, seed, counters, max_plies, over and history are its arguments, and the games its games -- with
    either table optional (None: neutral), whose draw books coef[b] times every candidate's share of every draw of row b.
    pos uint8 [B,192] with any B >= 1: one launch per BALANCE_MAX_ROWS rows.  coef: integers [B] on any device; a
    coefficient beyond BALANCE_MAX_COEF in magnitude is a ValueError before any launch, as is every other argument out of
    its domain.  grad_p, grad_t: None (zeroed here) or int64 [PATTERN_ENTRIES] / [TACTIC_ENTRIES] on the device of pos, added
    to; the sums of one launch stay below 2^61, and B * max_plies * max|coef| * 2^25 -- what all the launches of this call can
    add up to -- must stay below 2^63 (ValueError otherwise: split the rows); what the accumulators held before is the
    caller's to bound.
    -> (grad_p, grad_t, over uint8 [B], plies int32 [B], moves int16 [B,max_plies] or None, status int32 [B])."""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 2 or pos.shape[1] != POS_BYTES or pos.shape[0] < 1:
        raise ValueError(f"pos must be [B, {POS_BYTES}] with B >= 1")
    if coef is None:
        raise ValueError("coef must be integers [B]")
    B, dev, max_plies = int(pos.shape[0]), pos.device, int(max_plies)
    if not 1 <= max_plies <= MAX_PLAYOUT_PLIES:
        raise ValueError(f"max_plies must be 1..{MAX_PLAYOUT_PLIES}, got {max_plies}")
    pp, cp = _dev(pos, "pos", dtype=torch.uint8), _dev(counters, "counters", (B, 4), torch.int32)
    if counters.device != dev:
        raise ValueError("counters must be on the device of pos")
    tables = _weight_tables(pos, table, tactics)
    coef = balance_coef(coef, B, dev)
    top = int(coef.abs().max())
    if B * max_plies * top * (2 << BALANCE_Q) >= 2 ** 63:               # every launch adds into the same accumulators
        raise ValueError(f"{B} rows of {max_plies} plies with |coef| up to {top} could pass 2^63 in the accumulators: split the rows")
    if over is not None and over.device != dev:
        raise ValueError("over must be on the device of pos")
    over_p = None if over is None else _dev(over, "over", (B,), torch.uint8)
    for g, n, name in ((grad_p, PATTERN_ENTRIES, "grad_p"), (grad_t, TACTIC_ENTRIES, "grad_t")):
        if g is not None and (_dev(g, name, (n,), torch.int64) == 0 or g.device != dev):
            raise ValueError(f"{name} must be on the device of pos")
    grad_p = torch.zeros((PATTERN_ENTRIES,), dtype=torch.int64, device=dev) if grad_p is None else grad_p
    grad_t = torch.zeros((TACTIC_ENTRIES,), dtype=torch.int64, device=dev) if grad_t is None else grad_t
    if over is None:
        over = torch.zeros((B,), dtype=torch.uint8, device=dev)
        over_p = over.data_ptr()
    plies = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    moves = torch.empty((B, max_plies), dtype=torch.int16, device=dev) if history else None
    lib, stream, key = load(), _stream(pos), seed_u64(seed)
    for s in range(0, B, BALANCE_MAX_ROWS):
        n = min(BALANCE_MAX_ROWS, B - s)
        _check(lib.bkt_balance_sums(pp + s * POS_BYTES, n, key, cp + s * 16, *tables, coef.data_ptr() + s * 4, grad_p.data_ptr(),
                                    grad_t.data_ptr(), max_plies, over_p + s, plies.data_ptr() + s * 4,
                                    None if moves is None else moves.data_ptr() + s * max_plies * 2,
                                    status.data_ptr() + s * 4, stream), "bkt_balance_sums")
    return grad_p, grad_t, over, plies, moves, status

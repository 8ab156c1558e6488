"""-m gpu: one MM pass on the MI355X (bkt_mm_sums; bokego_amd/mmfit.py) against the numpy mirror, integer for
integer: rows built by hand at every seating of the kernel, split and repeated calls, the refused calls, and the packing and
the whole fit on both rules."""
import ctypes

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import lockstep as L
from bokego_amd import mmfit as M
from bokego_amd import patterns as PT
from bokego_amd import rollout as RO
from bokego_amd import tactics as TC
from test_mmfit_cpu import G_MAX, G_MIN, hand_rows, random_rows, strengths

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FIELDS = ("den_p", "den_t", "total", "chosen", "rank")


def device_sums(codes, moves, gp, gt):
    return M.sums(M.Packed(codes, moves, None, None), gp, gt, rules="device")


def same(dev, host, what):
    for f in FIELDS:
        d, h = getattr(dev, f), getattr(host, f)
        assert d.dtype == h.dtype and d.shape == h.shape, (what, f)
        assert np.array_equal(d, h), (what, f, np.nonzero(d != h)[0][:8])


# ---- 1. the kernel against the mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "low", "high", "low-high", "high-low"])
def test_sums_equal_the_mirror_at_every_seating(kind):
    """rows = 1, 3, 4, 7: a lone row, a full workgroup, a tail of one, and one past two workgroups; 3103: one round more than
    the grid has workgroups, so some walk two rounds."""
    torch.cuda.set_device(DEV)
    rng = np.random.default_rng(6)
    gp, gt = strengths(rng, kind)
    codes, moves = hand_rows()
    for rows in (1, 3, 4, 7):
        same(device_sums(codes[:rows], moves[:rows], gp, gt), M.sums_host(codes[:rows], moves[:rows], gp, gt), (kind, rows))
    order = [6, 1, 0]                                                   # the tie row and the colliding row at other seats
    same(device_sums(codes[order], moves[order], gp, gt), M.sums_host(codes[order], moves[order], gp, gt), (kind, order))
    if kind == "random":
        big = random_rows(rng, 3 * 1024 + 31)
        big[0][::5], big[1][::5] = codes[0], 40                         # the empty board's rows, all over the grid
        same(device_sums(*big, gp, gt), M.sums_host(*big, gp, gt), (kind, len(big[1])))


# ---- 2. calls add up, runs repeat ------------------------------------------------------------------------------------------------
def test_split_calls_add_up_and_runs_repeat():
    torch.cuda.set_device(DEV)
    rng = np.random.default_rng(7)
    gp, gt = strengths(rng)
    codes, moves = random_rows(rng, 50)
    codes[:7], moves[:7] = hand_rows()
    c, m = torch.from_numpy(codes.view(np.int32)).to(DEV), torch.from_numpy(moves).to(DEV)
    whole = T.mm_sums(c, m, gp, gt)
    again = T.mm_sums(c, m, gp, gt)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    den_p, den_t, total, chosen, rank = T.mm_sums(c[:20], m[:20], gp, gt)
    out = T.mm_sums(c[20:], m[20:], gp, gt, den_p, den_t)
    assert out[0] is den_p and out[1] is den_t
    assert torch.equal(den_p, whole[0]) and torch.equal(den_t, whole[1])
    for i, part in ((2, total), (3, chosen), (4, rank)):
        assert torch.equal(torch.cat([part, out[i]]), whole[i])
    host = M.sums_host(codes, moves, gp, gt)
    assert np.array_equal(whole[0].cpu().numpy().view(np.uint64), host.den_p) and host.den_p.any()


# ---- 3. refused calls --------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    torch.cuda.set_device(DEV)
    lib = T.load()
    gp, gt = (torch.from_numpy(g.astype(np.int64)).to(torch.int32).to(DEV) for g in strengths(np.random.default_rng(8)))
    codes, moves = hand_rows()
    c, m = torch.from_numpy(codes.view(np.int32)).to(DEV), torch.from_numpy(moves).to(DEV)
    outs = [torch.full((n,), -99, dtype=dt, device=DEV) for n, dt in ((PT.ENTRIES, torch.int64), (TC.ENTRIES, torch.int64),
                                                                      (7, torch.int64), (7, torch.int64), (7, torch.int32))]
    args = [c.data_ptr(), m.data_ptr(), 7, gp.data_ptr(), gt.data_ptr()] + [o.data_ptr() for o in outs]
    for hole in (0, 1, 3, 4, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[hole] = None
        assert lib.bkt_mm_sums(*bad, None) == -1, hole
    for rows in (0, -1, T.MM_MAX_ROWS + 1):
        bad = list(args)
        bad[2] = rows
        assert lib.bkt_mm_sums(*bad, None) == -1, rows
    torch.cuda.synchronize()
    assert all(bool((o == -99).all()) for o in outs)
    assert lib.bkt_mm_sums(*args, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)) == 0
    torch.cuda.synchronize()
    assert not bool((outs[4] == -99).any()) and bool((outs[0] != -99).any())
    # the binding: a strength outside the domain is refused before any launch
    good_p, good_t = strengths(np.random.default_rng(8))
    for value in (G_MIN - 1, G_MAX + 1):
        bad_p, bad_t = good_p.copy(), good_t.copy()
        bad_p[0], bad_t[63] = value, value
        den_p = torch.full((PT.ENTRIES,), 5, dtype=torch.int64, device=DEV)
        den_t = torch.full((TC.ENTRIES,), 5, dtype=torch.int64, device=DEV)
        for pair in ((bad_p, good_t), (good_p, bad_t)):
            with pytest.raises(ValueError, match="strength"):
                T.mm_sums(c, m, *pair, den_p, den_t)
        torch.cuda.synchronize()
        assert bool((den_p == 5).all()) and bool((den_t == 5).all())
    with pytest.raises(ValueError):
        T.mm_sums(c[:0], m[:0], good_p, good_t)
    with pytest.raises(ValueError):
        T.mm_sums(c, m[:6], good_p, good_t)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def test_pack_and_fit_agree_on_both_rules():
    """Six games of at most 40 plies, three iterations."""
    torch.cuda.set_device(DEV)
    start = L.initial_positions(6)
    fin = RO.random_playouts(start, 5, max_plies=40, rules="host")
    host, dev = M.pack(start, fin.moves, rules="host"), M.pack(start, fin.moves, rules="device", device=DEV)
    assert isinstance(dev.codes, torch.Tensor) and dev.codes.dtype == torch.int32 and dev.codes.device == DEV
    got = M.host(dev)
    assert got.codes.dtype == np.uint32 and got.codes.shape == host.codes.shape == (240, 81)
    for f in M.Packed._fields:
        assert np.array_equal(getattr(got, f), getattr(host, f)), f
    a, b = M.fit(dev, iterations=3, rules="device"), M.fit(host, iterations=3, rules="host")
    assert np.array_equal(a.gp, b.gp) and np.array_equal(a.gt, b.gt) and a.log == b.log
    assert len(a.log) == 7 and a.log[-1]["penalised_ll"] > a.log[0]["penalised_ll"] and (a.gt != M.G_ONE).any()
    # the tables under the draw itself, through the existing kernel and through its mirror
    table, tactics = M.tables(a.gp, a.gt)
    assert M.evaluate(start, fin.moves, table, tactics, device=DEV) == M.evaluate(start, fin.moves, table, tactics, rules="host")

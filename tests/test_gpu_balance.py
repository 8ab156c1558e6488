"""-m gpu: the gradient sums of simulation balancing on the MI355X (bkt_balance_sums; bokego_amd/balance.py)
against the numpy mirror, integer for integer: the rows built by hand at every seating of the kernel and with every table
set, the games against the kernels it wraps, calls that add up and repeat, the refused calls, and the gradient and the fit
on both rules."""

import numpy as np
import pytest
import torch

from bokego_amd import _trainlib as T
from bokego_amd import balance as B
from bokego_amd import lockstep as L
from bokego_amd import rollout as RO
from test_balance_cpu import HAND_COEF, SEED, hand_rows, random_rows, table_sets

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LIVE = [0, 1, 2, 3, 5]                                                 # the hand-built rows that are not over


def same(dev, host, what):
    for f in B.Sums._fields:
        d, h = getattr(dev, f), getattr(host, f)
        assert d.dtype == h.dtype and d.shape == h.shape, (what, f, d.dtype, h.dtype, d.shape, h.shape)
        assert np.array_equal(d, h), (what, f, np.argwhere(d != h)[:8])


def both(recs, ctr, coef, patterns, tactics, max_plies, over=None, seed=SEED):
    return (B.sums(recs, seed, ctr, coef, patterns, tactics, max_plies, rules="device", device=DEV, over=over),
            B.sums_host(recs, seed, ctr, coef, patterns, tactics, max_plies, over=over))


# ---- 1. the kernel against the mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["both", "patterns", "tactics", "none"])
def test_sums_equal_the_mirror_at_every_seating(name):
    """rows = 1, 3, 4, 6 of the hand-built set and 7 with a row repeated: a lone row, a full workgroup, a tail of one, two
    full workgroups, and one past them; then another seat order; max_plies 1, 8 and the default."""
    torch.cuda.set_device(DEV)
    patterns, tactics = table_sets()[name]
    recs, over, ctr = hand_rows()
    for rows in (1, 3, 4, 6):
        same(*both(recs[:rows], ctr[:rows], HAND_COEF[:rows], patterns, tactics, 8, over[:rows]), (name, rows))
    seven = [0, 1, 2, 3, 4, 5, 1]
    same(*both(recs[seven], ctr[seven], HAND_COEF[seven], patterns, tactics, 8, over[seven]), (name, 7))
    order = [5, 3, 0, 2, 4, 1]
    same(*both(recs[order], ctr[order], HAND_COEF[order], patterns, tactics, 8, over[order]), (name, order))
    for max_plies in (1, B.MAX_PLIES):
        dev, host = both(recs, ctr, HAND_COEF, patterns, tactics, max_plies, over)
        same(dev, host, (name, "max_plies", max_plies))
    assert dev.over[LIVE].all() and dev.grad_p.any() and dev.grad_t.any() and dev.grad_p.sum() == dev.grad_t.sum()


def test_many_rows_with_the_empty_board_all_over_the_grid():
    """3,103 rows, a third of them with a coefficient at an end of the range, the empty board at every fifth: the hot
    stone-free indices from every workgroup, and 1,035 workgroups' flushes into the same entries."""
    torch.cuda.set_device(DEV)
    patterns, tactics = table_sets()["both"]
    recs, ctr, coef = random_rows(3 * 1024 + 31)
    coef[::3] = np.where(np.arange(len(coef[::3])) % 2, B.MAX_COEF, -B.MAX_COEF)
    dev, host = both(recs, ctr, coef, patterns, tactics, 8)
    same(dev, host, "random rows")
    assert dev.grad_p[0] != 0 and np.count_nonzero(dev.grad_p) > 1000


# ---- 2. the games are untouched -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["both", "patterns", "tactics", "none"])
def test_the_games_are_those_of_the_kernel_it_wraps(name):
    torch.cuda.set_device(DEV)
    patterns, tactics = table_sets()[name]
    recs, ctr, coef = random_rows(100, seed=4)
    over0 = torch.zeros(100, dtype=torch.uint8, device=DEV)
    over0[7] = 1
    pos, c = torch.from_numpy(recs).to(DEV), torch.from_numpy(ctr).to(DEV)
    p, t = (None if x is None else x.device(DEV) for x in (patterns, tactics))
    for max_plies in (5, 400):
        mine, theirs = pos.clone(), pos.clone()
        got = T.balance_sums(mine, SEED, c, p, t, coef, max_plies, over=over0.clone())[2:]
        if tactics is not None:
            want = T.tactical_playouts(theirs, SEED, c, p, t, max_plies, over=over0.clone())
        elif patterns is not None:
            want = T.pattern_playouts(theirs, SEED, c, p, max_plies, over=over0.clone())
        else:
            want = T.random_playouts(theirs, SEED, c, max_plies, over=over0.clone())
        assert torch.equal(mine, theirs) and torch.equal(mine[7], pos[7])
        for a, b, what in zip(got, want, ("over", "plies", "moves", "status")):
            assert torch.equal(a, b), (name, max_plies, what)
        assert not got[3].any()
    if name == "none":                                                  # neutral tables are no tables
        from bokego_amd import patterns as PT
        from bokego_amd import tactics as TC
        neutral = T.balance_sums(pos.clone(), SEED, c, PT.PatternTable.constant(256).device(DEV), TC.TacticTable.neutral().device(DEV),
                                 coef, 400, over=over0.clone())
        assert all(torch.equal(a, b) for a, b in zip(neutral[2:], got))


# ---- 3. the accumulators -----------------------------------------------------------------------------------------------------------
def test_calls_add_up_and_runs_repeat():
    torch.cuda.set_device(DEV)
    patterns, tactics = table_sets()["both"]
    recs, ctr, coef = random_rows(50, seed=5)
    pos, c = torch.from_numpy(recs).to(DEV), torch.from_numpy(ctr).to(DEV)
    p, t = patterns.device(DEV), tactics.device(DEV)
    whole = T.balance_sums(pos.clone(), SEED, c, p, t, coef, 30)
    again = T.balance_sums(pos.clone(), SEED, c, p, t, coef, 30)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)) and whole[0].any()
    # into arrays that are not zero, in two calls over split rows
    rng = np.random.default_rng(1)
    base_p = torch.from_numpy(rng.integers(-2 ** 40, 2 ** 40, T.PATTERN_ENTRIES)).to(DEV)
    base_t = torch.from_numpy(rng.integers(-2 ** 40, 2 ** 40, T.TACTIC_ENTRIES)).to(DEV)
    gp, gt = base_p.clone(), base_t.clone()
    first = T.balance_sums(pos[:20].clone(), SEED, c[:20].contiguous(), p, t, coef[:20], 30, grad_p=gp, grad_t=gt)
    second = T.balance_sums(pos[20:].clone(), SEED, c[20:].contiguous(), p, t, coef[20:], 30, grad_p=gp, grad_t=gt)
    assert first[0] is gp and second[1] is gt
    assert torch.equal(gp - base_p, whole[0]) and torch.equal(gt - base_t, whole[1])
    for i in (2, 3, 4, 5):
        assert torch.equal(torch.cat([first[i], second[i]]), whole[i])
    host = B.sums_host(recs, SEED, ctr, coef, patterns, tactics, 30)
    assert np.array_equal(whole[0].cpu().numpy(), host.grad_p) and np.array_equal(whole[1].cpu().numpy(), host.grad_t)
    neg = T.balance_sums(pos.clone(), SEED, c, p, t, -coef, 30)
    assert torch.equal(neg[0], -whole[0]) and torch.equal(neg[1], -whole[1])


def test_refused_calls_write_nothing():
    torch.cuda.set_device(DEV)
    lib = T.load()
    patterns, tactics = table_sets()["both"]
    recs, over, ctr = hand_rows()
    pos, c = torch.from_numpy(recs).to(DEV), torch.from_numpy(ctr).to(DEV)
    p, t = patterns.device(DEV), tactics.device(DEV)
    coef = torch.from_numpy(HAND_COEF.astype(np.int32)).to(DEV)
    outs = dict(pos=pos.clone(), gp=torch.full((T.PATTERN_ENTRIES,), 77, dtype=torch.int64, device=DEV),
                gt=torch.full((T.TACTIC_ENTRIES,), 77, dtype=torch.int64, device=DEV),
                over=torch.zeros(6, dtype=torch.uint8, device=DEV), plies=torch.full((6,), 77, dtype=torch.int32, device=DEV),
                moves=torch.full((6, 8), 77, dtype=torch.int16, device=DEV), status=torch.full((6,), 77, dtype=torch.int32, device=DEV))
    before = {k: v.clone() for k, v in outs.items()}

    def call(batch=6, max_plies=8, **null):
        a = dict(pos=outs["pos"].data_ptr(), counters=c.data_ptr(), coef=coef.data_ptr(), gp=outs["gp"].data_ptr(),
                 gt=outs["gt"].data_ptr(), over=outs["over"].data_ptr(), plies=outs["plies"].data_ptr(), status=outs["status"].data_ptr())
        a.update({k: None for k in null})
        return lib.bkt_balance_sums(a["pos"], batch, SEED, a["counters"], p.data_ptr(), t.data_ptr(), a["coef"], a["gp"], a["gt"],
                                    max_plies, a["over"], a["plies"], outs["moves"].data_ptr(), a["status"], None)

    for kw in (dict(coef=1), dict(gp=1), dict(gt=1), dict(pos=1), dict(counters=1), dict(over=1), dict(plies=1), dict(status=1),
               dict(batch=0), dict(batch=-1), dict(batch=T.BALANCE_MAX_ROWS + 1), dict(max_plies=0),
               dict(max_plies=T.MAX_PLAYOUT_PLIES + 1)):
        assert call(**kw) == -1, kw                                     # BKT_ERR_ARG
    # the binding refuses before any launch
    for kw in (dict(coef=HAND_COEF + B.MAX_COEF), dict(coef=None), dict(coef=HAND_COEF[:5]), dict(max_plies=0),
               dict(max_plies=1025), dict(pos=outs["pos"][:0]), dict(grad_p=outs["gt"]), dict(counters=c[:5].contiguous())):
        a = {**dict(pos=outs["pos"], seed=SEED, counters=c, table=p, tactics=t, coef=HAND_COEF, max_plies=8, over=outs["over"],
                    grad_p=outs["gp"], grad_t=outs["gt"]), **kw}
        with pytest.raises(ValueError):
            T.balance_sums(**a)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, before[k]), k
    assert call() == 0                                                  # and the same call with nothing missing runs
    torch.cuda.synchronize()
    assert not torch.equal(outs["gp"], before["gp"]) and (outs["plies"] != 77).all()


# ---- 4. the driver: device against host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six_positions():
    recs = RO.random_playouts(L.initial_positions(6), 3, max_plies=40, rules="host").records
    return recs, np.array([1.0, -1.0, 0.5, -0.25, 1.0, -1.0])


def test_gradient_on_the_device_equals_the_host(six_positions):
    torch.cuda.set_device(DEV)
    recs, targets = six_positions
    patterns, tactics = table_sets()["small"]
    dev, host = (B.gradient(recs, targets, patterns, tactics, 4, 3, 5, rules=rules) for rules in ("device", "host"))
    for f in B.Gradient._fields:
        assert np.array_equal(getattr(dev, f), getattr(host, f)), f
    assert dev.grad_p.any() and dev.grad_t.any()


def test_fit_on_the_device_equals_the_host(six_positions):
    torch.cuda.set_device(DEV)
    recs, targets = six_positions
    kw = dict(iterations=2, lr=4.0, M=4, N=3, seed=2, held_out=(recs[:3], targets[:3]))
    dev, host = (B.fit(recs, targets, rules=rules, **kw) for rules in ("device", "host"))
    assert np.array_equal(dev.gp, host.gp) and np.array_equal(dev.gt, host.gt) and dev.log == host.log
    assert np.array_equal(dev.patterns.array, host.patterns.array) and np.array_equal(dev.tactics.array, host.tactics.array)
    assert (dev.gt != 65536).any()
    e_dev, e_host = (B.value_error(recs, targets, dev.patterns, dev.tactics, 8, 1, rules=rules) for rules in ("device", "host"))
    assert e_dev == e_host

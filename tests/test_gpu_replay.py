"""-m gpu: the device walker of bokego_amd/replay.py against the host walker on test_replay_cpu.py's seven games at batches of
three -- the smallest set with a remainder batch, an empty game and a trailing pass -- and what the fitting modules compute
through it on the device against the pins of the host rules."""
import json

import numpy as np
import pytest
import torch

from bokego_amd import mmfit as M
from bokego_amd import patterns as PT
from bokego_amd import replay as R
from bokego_amd import tactics as TC
from test_replay_cpu import EVAL_PLIES, LENGTHS, PINS, digest, game_set, tables

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


def test_the_device_walker_yields_what_the_host_walker_yields():
    start, moves = R.check_games(*game_set())
    host = {(first, k): (live, recs.copy(), mv, ok) for k, first, live, recs, mv, ok in R.replay_host(start, moves, 3)}
    seen = []
    for k, first, pos, mv, live, ok in R.replay_device(start, moves, DEV, 3):
        seen.append((first, k))
        assert pos.device == mv.device == live.device == ok.device == DEV and mv.dtype == torch.int32 and ok.dtype == torch.uint8
        assert np.array_equal(mv.cpu().numpy(), moves[first:first + 3, k])
        rows = np.nonzero(live.cpu().numpy())[0]
        if (first, k) not in host:                                    # a ply the host walker skips: no game of the batch is live
            assert len(rows) == 0
            continue
        h_live, h_recs, h_mv, h_ok = host[first, k]
        assert np.array_equal(rows, h_live) and np.array_equal(pos.cpu().numpy(), h_recs), (first, k)
        assert np.array_equal(ok.cpu().numpy()[rows] != 0, h_ok), (first, k)
    assert seen == [(first, k) for first in (0, 3, 6) for k in range(max(LENGTHS))]       # every ply of every batch, in order
    assert set(host) <= set(seen) and (0, 30) not in host and (3, 44) in host
    bare = [ok for _, _, _, _, _, ok in R.replay_device(start, moves, DEV, 3, playable=False)]
    assert len(bare) == len(seen) and all(ok is None for ok in bare)


def test_the_integers_of_the_fits_equal_the_pins(pins):
    start, moves = game_set()
    assert [digest(a) for a in PT.counts(start, moves, device=DEV)] == pins["patterns.counts"]
    packed = M.pack(start, moves, device=DEV)
    assert isinstance(packed.codes, torch.Tensor) and packed.codes.dtype == packed.moves.dtype == torch.int32
    assert [digest(a) for a in M.host(packed)] == pins["mmfit.pack"]


@pytest.mark.parametrize("name, with_table", [("tactics.counts", False), ("tactics.counts(patterns)", True)])
def test_the_mass_equals_the_pinned_host_mass(pins, name, with_table):
    start, moves = game_set()
    mass_h = np.frombuffer(bytes.fromhex(pins[name][2]), np.float64)
    mass_d, played_d = TC.counts(start, moves, tables()[0] if with_table else None, device=DEV)
    assert digest(played_d) == pins[name][1] and mass_d.dtype == np.float64 and mass_d.shape == mass_h.shape == (TC.ENTRIES,)
    err = np.abs(mass_d - mass_h) / np.maximum(np.abs(mass_h), 1e-300)
    print("mass: largest relative difference", err[mass_h > 0].max())
    assert ((mass_h > 0) == (mass_d > 0)).all() and (err[mass_h > 0] <= 1e-8).all()         # test_gpu_tactics.py's tolerance


@pytest.mark.parametrize("plies", [None, EVAL_PLIES])
def test_evaluate_is_the_same_on_both_rules(plies):
    start, moves = game_set()
    table, tac = tables()
    got = M.evaluate(start, moves, table, tac, device=DEV, plies=plies)
    assert got == M.evaluate(start, moves, table, tac, rules="host", plies=plies) and got["moves"] > 0


@pytest.mark.parametrize("cls", [PT.PatternTable, TC.TacticTable])
def test_a_table_keeps_one_copy_per_device(cls):
    table = cls(np.random.default_rng(6).integers(0, 65536, cls.ENTRIES).astype(np.uint16))
    torch.cuda.set_device(DEV)
    d = table.device(DEV)
    assert d.device == DEV and d.dtype == torch.int16 and np.array_equal(d.cpu().numpy().view(np.uint16), table.array)
    assert table.device("cuda") is d and table.device("cuda:0") is d and table.device(DEV) is d
    assert cls(table.array).device(DEV) is not d                                          # the cache is the table's own

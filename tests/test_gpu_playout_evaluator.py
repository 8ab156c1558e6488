"""-m gpu: PlayoutEvaluator and the playout_* functions on the MI355X through public names only -- every combination of the
evaluator's opt-in terms against the host mirror bit for bit, and the launches each of them makes, counted.  Five records
and 5 playouts: the AMAF kernels end on a round of one wave and the owner kernel on one of two seats.  The counts are the
contract of rollout.py's one playout run: no term may cost a launch it did not cost before."""
import itertools

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import rollout as RO
from test_amaf_cpu import _FakeEngine, seeded_tables
from test_gpu_amaf import five  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

PLAYOUTS, SEED, N_POLICY = 5, 9, 3
LAUNCHES = ("random_playouts", "pattern_playouts", "tactical_playouts", "area_score", "amaf_counts", "amaf_counts_sides",
            "owner_counts", "move_weights")
# (prior, rave, criticality, pattern_prior, n_policy): the eight combinations of the terms at prior=1, and the plain value
COMBINATIONS = [(1.0, rave, gamma, mu, N_POLICY) for rave, gamma, mu in itertools.product((False, True), (0.0, 0.5), (0.0, 1.5))]
COMBINATIONS.append((0.0, False, 0.0, 0.0, 0))


def evaluator(rules, prior, rave, gamma, mu):
    pat, tac = seeded_tables()
    more = dict(prior_patterns=pat, prior_tactics=tac) if mu else {}
    return RO.PlayoutEvaluator(None if prior == 1.0 else _FakeEngine(), PLAYOUTS, seed=SEED, rules=rules, prior=prior, rave=rave,
                               criticality=gamma, pattern_prior=mu, **more)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("prior,rave,gamma,mu,n_policy", COMBINATIONS)
def test_the_device_rules_equal_the_host_rules_bit_for_bit(five, prior, rave, gamma, mu, n_policy):  # noqa: F811
    dev, host = (ev.finish(ev.submit(five, n_policy), normalise=lambda x: x)
                 for ev in (evaluator(rules, prior, rave, gamma, mu) for rules in ("device", "host")))
    assert len(dev) == len(host) == 2 + rave
    assert dev[0].shape == (n_policy, 81) and dev[1].shape == (5,) and dev[0].dtype == dev[1].dtype == np.float32
    assert same_bits(dev[0], host[0]) and same_bits(dev[1], host[1])
    if rave:
        assert dev[2][0] == host[2][0] == PLAYOUTS
        assert all(same_bits(d, h) and d.dtype == np.int32 for d, h in zip(dev[2][1:], host[2][1:]))
        assert dev[2][2].shape == dev[2][3].shape == (5, 2, 81) and dev[2][1].shape == (5,)


@pytest.fixture
def launches(monkeypatch):
    """Wrap the launches of _trainlib -> {name: [the history= of each call, None where the launch has none]}."""
    seen = {name: [] for name in LAUNCHES}

    def counted(name, fn):
        def call(*args, **kw):
            seen[name].append(kw.get("history"))
            return fn(*args, **kw)
        return call

    for name in LAUNCHES:
        monkeypatch.setattr(T, name, counted(name, getattr(T, name)))
    return seen


def taken(seen):
    """The launches since the last look -> ({name: calls} without the zeros, the history= of the playout launches)."""
    counts = {name: len(calls) for name, calls in seen.items() if calls}
    history = [h for name in LAUNCHES[:3] for h in seen[name]]
    for calls in seen.values():
        calls.clear()
    return counts, history


def test_the_launches_of_every_combination_and_function(five, launches):  # noqa: F811
    for prior, rave, gamma, mu, n_policy in COMBINATIONS:
        ev = evaluator("device", prior, rave, gamma, mu)
        ev.finish(ev.submit(five, n_policy))
        want = {"random_playouts": 1, "area_score": 1}
        if rave:
            want["amaf_counts_sides"] = 1
        elif prior:
            want["amaf_counts"] = 1
        if gamma:
            want["owner_counts"] = 1
        if mu:
            want["move_weights"] = 1
        assert taken(launches) == (want, [bool(rave or prior)]), (prior, rave, gamma, mu)
    pat, tac = seeded_tables()
    RO.playout_value(five, PLAYOUTS, SEED)
    assert taken(launches) == ({"random_playouts": 1, "area_score": 1}, [False])
    RO.playout_value(five, PLAYOUTS, SEED, patterns=pat)
    assert taken(launches) == ({"pattern_playouts": 1, "area_score": 1}, [False])
    RO.playout_value(five, PLAYOUTS, SEED, patterns=pat, tactics=tac)
    assert taken(launches) == ({"tactical_playouts": 1, "area_score": 1}, [False])
    RO.playout_amaf(five, PLAYOUTS, SEED, sides=1)
    assert taken(launches) == ({"random_playouts": 1, "area_score": 1, "amaf_counts": 1}, [True])
    RO.playout_amaf(five, PLAYOUTS, SEED, sides=2)
    assert taken(launches) == ({"random_playouts": 1, "area_score": 1, "amaf_counts_sides": 1}, [True])
    RO.playout_ownership(five, PLAYOUTS, SEED)
    assert taken(launches) == ({"random_playouts": 1, "owner_counts": 1}, [False])    # no bkt_area_score
    RO.playout_ownership(five, PLAYOUTS, SEED, tactics=tac)
    assert taken(launches) == ({"tactical_playouts": 1, "owner_counts": 1}, [False])

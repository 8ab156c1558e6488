"""CPU: PlayoutEvaluator over the whole product of its options on the host rules, bit for bit against recorded results.

The product is prior x rave x criticality x pattern_prior x playout tables x n_policy on test_amaf_cpu's three records, 3
playouts, seed 4: 144 combinations, of which 108 construct and 36 -- a prior term without a prior -- are refused.  What
submit hands to finish is private to the evaluator; what finish returns is not, and tests/golden/playout_evaluator_matrix.npz
holds it for every combination: probs, values and, with rave, the records.  The fixture was recorded on commit 6680277, the
last one whose evaluator passed its requests on as positional tuples, by this module's own switch:

    python tests/test_playout_evaluator_matrix_cpu.py --record

It holds results only, and is rewritten only when the search is meant to compute something else.
"""
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from bokego_amd import rollout as RO
from test_amaf_cpu import _FakeEngine, seeded_tables, three_records

FIXTURE = os.path.join(GOLDEN, "playout_evaluator_matrix.npz")
PLAYOUTS, SEED = 3, 4
PRODUCT = list(itertools.product((0.0, 0.5, 1.0), (False, True), (0.0, 0.5), (0.0, 1.5), (False, True), (0, 2, 3)))
FIELDS = ("probs", "values", "playouts", "wins", "played", "won_at")


def key_of(prior, rave, gamma, mu, tables, n_policy):
    return f"prior{prior:g}_rave{int(rave)}_crit{gamma:g}_pp{mu:g}_tables{int(tables)}_n{n_policy}"


def run_matrix():
    """-> ({key + "/" + field: array} of the combinations that construct, the keys of those refused with ValueError)."""
    recs = three_records()
    pat, tac = seeded_tables()
    results, refused = {}, []
    for prior, rave, gamma, mu, tables, n_policy in PRODUCT:
        key = key_of(prior, rave, gamma, mu, tables, n_policy)
        kw = dict(seed=SEED, rules="host", prior=prior, rave=rave, criticality=gamma, pattern_prior=mu,
                  prior_patterns=pat if mu else None)
        if tables:
            kw.update(patterns=pat, tactics=tac)
        try:
            ev = RO.PlayoutEvaluator(None if prior == 1.0 else _FakeEngine(), PLAYOUTS, **kw)
        except ValueError:
            refused.append(key)
            continue
        out = ev.finish(ev.submit(recs, n_policy), normalise=lambda x: x)
        assert len(out) == 2 + rave, key
        results[key + "/probs"], results[key + "/values"] = out[0], out[1]
        if rave:
            results[key + "/playouts"] = np.asarray(out[2][0])
            results[key + "/wins"], results[key + "/played"], results[key + "/won_at"] = out[2][1:]
    return results, refused


@pytest.fixture(scope="module")
def matrix():
    return run_matrix()


def test_the_prior_terms_without_a_prior_are_refused_and_nothing_else(matrix):
    results, refused = matrix
    want = [key_of(*c) for c in PRODUCT if c[0] == 0.0 and (c[2] > 0.0 or c[3] > 0.0)]
    assert len(PRODUCT) == 144 and len(want) == 36 and refused == want
    assert refused == np.load(FIXTURE)["refused"].tolist()
    assert len({k.split("/")[0] for k in results}) == 108


def test_every_result_equals_the_recorded_one_bit_for_bit(matrix):
    results, _ = matrix
    with np.load(FIXTURE) as gold:
        assert sorted(results) == sorted(k for k in gold.files if k != "refused")
        compared = set()
        for k, got in results.items():
            want = gold[k]
            assert got.dtype == want.dtype and got.shape == want.shape, k
            assert got.tobytes() == want.tobytes(), k
            compared.add(k.split("/")[0])
    assert len(compared) == 108
    shapes = {k.split("/")[1]: results[k] for k in results if k.startswith(key_of(1.0, True, 0.5, 1.5, True, 2) + "/")}
    assert sorted(shapes) == sorted(FIELDS) and shapes["probs"].shape == (2, 81) and shapes["played"].shape == (3, 2, 81)
    assert shapes["probs"].dtype == shapes["values"].dtype == np.float32 and shapes["wins"].dtype == np.int32


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_playout_evaluator_matrix_cpu.py --record")
    results, refused = run_matrix()
    np.savez_compressed(FIXTURE, refused=np.array(refused), **results)
    print(f"{FIXTURE}: {len(results)} arrays of {len({k.split('/')[0] for k in results})} combinations, {len(refused)} refused, "
          f"{os.path.getsize(FIXTURE)} bytes")

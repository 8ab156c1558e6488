"""The hand-built corpus of adversarial_boards.py on the CPU: that it has the properties it was built for, that the host
rules (libbkgo) give the reference's recorded answers on it (tests/golden/adversarial_boards.npz, written by
tools/gen_adversarial_golden.py), and that the Python mirrors the GPU tests compare against agree with the C functions
wherever both exist on the same record.  The host is the oracle of test_gpu_adversarial_boards.py; this is its check."""
import ctypes
import os

import numpy as np
import pytest

import adversarial_boards as A
from bokego_amd import go
from bokego_amd import lockstep as L
from bokego_amd import rollout as RO
from conftest import GOLDEN

_PP = ctypes.POINTER(go.Pos)
STATUS = {0: 0, -11: 1, -12: 2, -13: 3}                                  # bk_pos_play's codes as the fixture's outcomes


@pytest.fixture(scope="module")
def corpus():
    return A.corpus()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "adversarial_boards.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_corpus_has_the_properties_it_was_built_for():
    C = A.check_conditions()
    assert len(C.recs) >= 500


def test_the_fixture_is_the_corpus(corpus, golden):
    kept = golden["kept"]
    assert golden["names"].tolist() == [corpus.names[i] for i in kept]
    assert np.array_equal(golden["records"], corpus.recs[kept])
    named = [i for i, n in enumerate(corpus.names) if not n.startswith("dense")]
    assert set(named) <= set(kept.tolist()), "only dense random boards may be left out of the fixture"
    assert len(kept) >= len(named) + 2 * A.DENSE_EACH * 2
    assert os.path.getsize(os.path.join(GOLDEN, "adversarial_boards.npz")) <= 256 * 1024


def test_host_rules_equal_the_reference(corpus, golden):
    lib = go.golib()
    buf = (ctypes.c_uint8 * 81)()
    plays = quirks = 0
    for row, i in enumerate(golden["kept"].tolist()):
        name = corpus.names[i]
        rec = corpus.recs[i].copy()
        p = ctypes.cast(rec.ctypes.data, _PP)
        # the legal-move list, before anything refreshes the cache (it does not depend on it)
        lib.bk_pos_legal_moves(p, buf)
        legal = np.frombuffer(buf, np.uint8).copy()
        ref_legal = golden["legal"][row]
        ref_planes = golden["planes"][row]
        ko = int(p.contents.ko)
        planes = np.empty((27, 81), np.uint8)
        scratch = rec.copy()
        lib.bk_pos_features_u8(ctypes.cast(scratch.ctypes.data, _PP), planes.ctypes.data, 0)
        if ko >= 0 and ref_legal[ko]:
            # Game.get_legal_moves never looks at a point of an empty region of two or more points: it takes the whole
            # region as legal, a ko point in it too, and features() then fills planes 5 and 13..26 there.  play_move
            # refuses the point (the outcome below), and no game sets a ko in such a region: the captured stone's other
            # neighbours were stones.  The host follows play_move: nothing at the ko point; every other value is compared.
            quirks += 1
            assert golden["outcome"][row][ko] == 1 and not legal[ko], name
            assert not planes[5, ko] and not planes[13:27, ko].any(), name
            ref_legal, ref_planes = ref_legal.copy(), ref_planes.copy()
            ref_legal[ko] = 0
            ref_planes[5, ko] = 0
            ref_planes[13:27, ko] = 0
        assert np.array_equal(legal, ref_legal), name
        bad = np.nonzero((planes != ref_planes).any(1))[0]
        assert len(bad) == 0, (name, bad)
        scratch = rec.copy()
        lib.bk_pos_liberties(ctypes.cast(scratch.ctypes.data, _PP), buf)
        assert np.array_equal(np.frombuffer(buf, np.uint8), golden["liberties"][row]), name
        assert np.float32(lib.bk_pos_score(p, 5.5)) == golden["score"][row], name
        captured = np.unpackbits(golden["captured"][row], axis=1)[:, :81].astype(bool)
        mover = 2 if p.contents.turn & 1 else 1
        for m in range(81):
            after = rec.copy()
            rc = lib.bk_pos_play(ctypes.cast(after.ctypes.data, _PP), m)
            plays += 1
            assert STATUS[rc] == golden["outcome"][row][m], (name, m, rc)
            if rc:
                assert np.array_equal(after, rec), (name, m)
                continue
            want = rec[:81].copy()
            want[m] = mover
            want[captured[m]] = 0
            assert np.array_equal(after[:81], want), (name, m)
            assert int(after[A.OFF_KO:A.OFF_KO + 2].view(np.int16)[0]) == golden["ko"][row][m], (name, m)
    assert plays == 81 * len(golden["kept"]) >= 81 * 400
    assert quirks <= 14, "only the records with a ko set by hand in an open region may differ there"


def test_python_mirrors_equal_the_c_functions(corpus):
    lib = go.golib()
    recs = corpus.recs.copy()
    buf = (ctypes.c_uint8 * 81)()
    playable, legal = RO.playable_host(recs), RO.legal_host(recs)
    owner, area = RO.owner_host(recs), L.area_score_host(recs, 5.5)
    planes = np.empty((len(recs), 27, 81), np.uint8)
    scratch = recs.copy()
    lib.bk_features_batch_u8(scratch.ctypes.data, len(recs), 192, planes.ctypes.data, 0)
    assert np.array_equal(recs, corpus.recs)                            # the mirrors only read
    empty_sets = 0
    for i in range(len(recs)):
        p = ctypes.cast(recs[i].ctypes.data, _PP)
        lib.bk_pos_legal_moves(p, buf)
        mover = 2 if p.contents.turn & 1 else 1
        want = [bool(buf[s]) and lib.bk_pos_possible_eye(p, s) != mover for s in range(81)]
        assert playable[i].tolist() == want, corpus.names[i]
        assert legal[i].tolist() == [bool(buf[s]) for s in range(81)], corpus.names[i]
        assert np.array_equal(legal[i], planes[i, L.LEGAL_PLANE] != 0), corpus.names[i]
        # Tromp-Taylor area from the Python flood: the C function's float, bit for bit
        black, white = int((owner[i] > 0).sum()), int((owner[i] < 0).sum())
        assert np.float32(area[i]) == np.float32(black) - (np.float32(white) + np.float32(5.5)), corpus.names[i]
        assert np.float32(lib.bk_pos_area_score(p, 5.5)) == np.float32(area[i])
        empty_sets += not playable[i].any()
    assert empty_sets >= 8, "the corpus holds sides without a playable point"
    one = (playable.sum(1) == 1).sum()
    assert one >= 8, "... and sides with exactly one"


def test_python_mirrors_run_the_corpus(corpus):
    """The mirrors of the code tables and of a whole playout accept every record (the GPU tests compare against them)."""
    from bokego_amd import patterns as PT
    from bokego_amd import tactics as TC
    recs = corpus.recs.copy()
    pc, tc = PT.codes_host(recs), TC.codes_host(recs)
    assert pc.shape == tc.shape == (len(recs), 81) and pc.min() >= 0 and pc.max() < PT.ENTRIES
    assert tc.min() >= 0 and tc.max() < TC.ENTRIES
    w = RO.move_weights_host(recs)
    assert np.array_equal(w != 0, RO.playable_host(recs))
    fin = RO.random_playouts(recs, 9, max_plies=8, rules="host")
    first = fin.moves[:, 0]
    for name, at in (("cap80_centre/b", 40), ("cap80_corner/b", 0), ("checker/b", 40)):
        assert first[A.index(name)] == at
    for name in ("cap80_centre/w", "cap80_corner/w", "checker/w"):
        assert first[A.index(name)] == go.PASS
    assert np.array_equal(recs, corpus.recs)

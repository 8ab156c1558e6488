"""CPU: RAVE in the native tree search and the two-sided AMAF counts it is fed with, as far as they need no GPU
-- the declaration and the binding of bkt_amaf_counts_sides, its host mirror against counts written out by hand, the
tree's backup rule against a pure-Python model keyed by position, the blended selection on a hand-made node, the searches
that must equal RAVE off, what bk_pool_set_rave refuses, snapshots, the whole search on the host rules, the keywords and
the command lines, and the kernel's resources when compiled for gfx950."""
import copy
import ctypes
import os
import pickle
import re
import subprocess
import zlib

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go, gtp, match, selfplay
from bokego_amd import rollout as RO
from bokego_amd.mcts_native import NativeMCTS, Position
from conftest import REPO
from test_amaf_cpu import BOARD, HAND_MOVES, HAND_PLAYED, HAND_WON, HAND_WON_AT

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
PASS, NONE = go.PASS, RO.MOVE_NONE

# The opponent's half of test_amaf_cpu's hand histories (records = 2, playouts = 3, max_plies = 8; odd plies are the
# opponent's, and the opponent wins the rows with won == 0), row by row:
#   record 0  row 0 (won)   7 at ply 1: the opponent's first, and it lost.  5 and 9 are the mover's.
#             row 1         nothing.
#             row 2 (lost)  1, 3, 5 and 80 at the plies 1, 3, 5, 7: the opponent's, and it won.  (5 is the mover's in row 0
#                           and the opponent's here: a point counts once per ROW.)
#   record 1  row 3 (lost)  40 at ply 0 is the mover's, -3 ends the row at ply 2: nothing.
#             row 4 (won)   40 at ply 1 and 7 at ply 7 are the opponent's, and it lost; 41 and 80 are the mover's.
#             row 5 (won)   41 at ply 1 is the opponent's, and it lost; 12 was first played at ply 4, by the mover.
HAND_PLAYED_1 = np.zeros((2, 81), np.int32)
HAND_WON_AT_1 = np.zeros((2, 81), np.int32)
HAND_PLAYED_1[0, [7, 1, 3, 5, 80]] = 1
HAND_WON_AT_1[0, [1, 3, 5, 80]] = 1
HAND_PLAYED_1[1, [40, 7, 41]] = 1


# ---- 1. the mirror ----------------------------------------------------------------------------------------------------------------
def test_host_counts_of_both_sides_equal_the_hand_written_ones():
    played, won_at = RO.amaf_counts_sides_host(HAND_MOVES, HAND_WON, 2, 3)
    assert played.dtype == won_at.dtype == np.int32 and played.shape == won_at.shape == (2, 2, 81)
    assert np.array_equal(played[:, 1], HAND_PLAYED_1), np.nonzero(played[:, 1] != HAND_PLAYED_1)
    assert np.array_equal(won_at[:, 1], HAND_WON_AT_1), np.nonzero(won_at[:, 1] != HAND_WON_AT_1)
    assert np.array_equal(played[:, 0], HAND_PLAYED) and np.array_equal(won_at[:, 0], HAND_WON_AT)
    p0, w0 = RO.amaf_counts_host(HAND_MOVES, HAND_WON, 2, 3)
    assert np.array_equal(played[:, 0], p0) and np.array_equal(won_at[:, 0], w0)
    assert (played.sum(1) <= 3).all() and (won_at <= played).all() and (won_at >= 0).all()
    # the same rows as six records of one playout each: nothing crosses a row
    p1, w1 = RO.amaf_counts_sides_host(HAND_MOVES, HAND_WON, 6, 1)
    assert np.array_equal(p1.reshape(2, 3, 2, 81).sum(1), played) and np.array_equal(w1.reshape(2, 3, 2, 81).sum(1), won_at)
    for bad in ((HAND_MOVES, HAND_WON, 3, 3), (HAND_MOVES, HAND_WON[:5], 2, 3), (HAND_MOVES, HAND_WON, 0, 3),
                (HAND_MOVES[0], HAND_WON, 2, 3)):
        with pytest.raises(ValueError):
            RO.amaf_counts_sides_host(*bad)


def junk_histories(rng, records, playouts, max_plies):
    """Random histories with the entries of test_gpu_amaf's test_any_history_gives_the_mirrors_counts: points, passes, end
    markers, entries above 80 and below BKT_MOVE_NONE."""
    rows = records * playouts
    moves = rng.integers(0, 81, (rows, max_plies)).astype(np.int16)
    junk = rng.random((rows, max_plies))
    moves[junk < 0.10] = PASS
    moves[(junk >= 0.10) & (junk < 0.14)] = 81
    moves[(junk >= 0.14) & (junk < 0.16)] = 32767
    moves[(junk >= 0.16) & (junk < 0.17)] = -32768
    moves[(junk >= 0.17) & (junk < 0.18)] = -3
    for r in range(rows):                                                 # most rows end somewhere, as playouts do
        if rng.random() < 0.7:
            moves[r, rng.integers(0, max_plies):] = NONE
    return moves, rng.integers(0, 2, rows).astype(np.uint8) * rng.integers(1, 256, rows).astype(np.uint8)


def test_side_0_of_any_history_is_the_one_sided_count():
    rng = np.random.default_rng(5)
    for records, playouts, max_plies in ((3, 9, 37), (7, 4, 101), (2, 6, 3), (1, 5, 1)):
        moves, won = junk_histories(rng, records, playouts, max_plies)
        played, won_at = RO.amaf_counts_sides_host(moves, won, records, playouts)
        p0, w0 = RO.amaf_counts_host(moves, won, records, playouts)
        assert np.array_equal(played[:, 0], p0) and np.array_equal(won_at[:, 0], w0)
        assert (played.sum(1) <= playouts).all() and (won_at <= played).all()
        # a row the opponent wins is one with won == 0: flipping every won swaps nothing but the wins
        pf, wf = RO.amaf_counts_sides_host(moves, (won == 0).astype(np.uint8), records, playouts)
        assert np.array_equal(pf, played) and np.array_equal(wf, played - won_at)


# ---- 2. header, library, Makefile, kernel ---------------------------------------------------------------------------------------
def test_header_binding_and_build_name_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src) and T.BKT_ABI_VERSION == 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bkt_amaf_counts_sides\s*\(\s*const\s+int16_t\s*\*\s*moves\s*,\s*int\s+max_plies\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*won\s*,\s*int\s+records\s*,\s*int\s+playouts\s*,"
                     r"\s*int32_t\s*\*\s*played\s*,\s*int32_t\s*\*\s*won_at\s*,\s*void\s*\*\s*stream\s*\)", code)
    comment = re.sub(r"\s*\n \*\s*", " ", src[:src.index("int bkt_amaf_counts_sides")].rsplit("/*", 1)[1])
    for phrase in ("side k & 1", "side 0 is the side to move at the record", "won[row] == 0", "[records, 2, 81]",
                   "side 0 equals bkt_amaf_counts' output", "BKT_ERR_ARG"):
        assert phrase in comment, phrase
    assert T.SYMBOLS["bkt_amaf_counts_sides"] == T.SYMBOLS["bkt_amaf_counts"] and callable(T.amaf_counts_sides)
    assert "amaf_counts_sides_host" in RO.__all__ and all(hasattr(RO, name) for name in RO.__all__)
    if os.path.exists(T.LIB_PATH):
        lib = ctypes.CDLL(T.LIB_PATH)
        assert lib.bkt_abi_version() == 4 and lib.bkt_amaf_counts_sides and lib.bkt_amaf_counts
    make = open(os.path.join(CSRC, "Makefile")).read()
    (line,) = [l for l in make.splitlines() if l.startswith("\t") and "-o $@" in l and "bk_playout_pat.hip" in l]
    assert "bk_playout_rave.hip" in line.split() and "bk_playout_amaf.hip" in line.split()
    (rule,) = [l for l in make.splitlines() if l.startswith("$(TRAIN_OUT):")]
    assert "bk_playout_rave.hip" in rule.split()
    for name in ("bk_playout.hip", "bk_playout_mc.hip", "bk_playout_pat.hip", "bk_playout_tac.hip", "bk_playout_amaf.hip"):
        assert "bk_playout_rave" not in open(os.path.join(CSRC, name)).read()
    # the tree's side: three new symbols, no struct and no version moved (tests/test_abi.py pins the sizes)
    tree = selfplay.treelib()
    for name in ("bk_pool_set_rave", "bk_pool_deliver_rave", "bk_pool_node_rave"):
        assert name in selfplay.TREE_SYMBOLS and hasattr(tree, name)
    assert tree.bk_go_abi_version() == 6 and ctypes.sizeof(selfplay.SearchParams) == 104


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_kernel_builds_alone_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout_rave.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"Function Name: ", r.stderr)[1:]
    assert len(blocks) == 1 and "amaf_counts_sides_kernel" in blocks[0].split()[0], [b.split()[0] for b in blocks]
    field = lambda pat: int(re.search(pat + r": (\d+)", blocks[0]).group(1))  # noqa: E731
    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field(r"SGPRs Spill") == 0 and field(r"VGPRs Spill") == 0, blocks[0]
    # two staging buffers of 4 rows x 1024 int16 and the waves' partial counts, now of two sides
    assert field(r"LDS Size \[bytes/block\]") == 2 * 4 * 1024 * 2 + 4 * 4 * 81 * 4, blocks[0]
    assert field(r" VGPRs") <= 64, blocks[0]


# ---- 3. the tree against a Python model -------------------------------------------------------------------------------------------
PLAYOUTS = 8
# A black wall on the left, a white one on the right, five empty points between them: 4, 22, 40, 58, 76.  Few moves, so 60
# rollouts go deep; FOUR are the points the scripted priors send black (4, 58) and white (22, 76) to.
NARROW = "".join("XXXX.OOOO" if r % 2 == 0 else "XXXXXOOOO" for r in range(9))
FOUR = (4, 22, 58, 76)


def pos_key(rec):
    """(board, ko, last move, side): what makes two positions one node (go.Game.key) -- from a 192-byte record."""
    rec = np.ascontiguousarray(rec, np.uint8)
    return bytes(rec[:81]) + bytes(rec[164:168]) + bytes([rec[172] & 1])


def scripted_record(key):
    """Seeded integers for one position: (wins, played [2,81], won_at [2,81]) of PLAYOUTS playouts, within what a real
    record can hold: played[0] + played[1] <= PLAYOUTS, won_at <= played."""
    rng = np.random.default_rng(zlib.crc32(key))
    wins = int(rng.integers(0, PLAYOUTS + 1))
    both = rng.integers(0, PLAYOUTS + 1, 81)
    played = np.zeros((2, 81), np.int32)
    played[0] = rng.integers(0, both + 1)
    played[1] = both - played[0]
    won_at = rng.integers(0, played + 1).astype(np.int32)
    return wins, played, won_at


class Scripted:
    """An evaluator of position records: priors that send black to FOUR[0] or FOUR[2], evenly, and white to FOUR[1] and then
    to FOUR[3] -- a narrow tree in which a,b,c,d and c,b,a,d meet in one node -- and value and AMAF record from
    scripted_record."""

    def __init__(self, records=True):
        self.records = records

    def __call__(self, recs, npol):
        B = len(recs)
        probs = np.full((npol, 81), 0.02 / 79, np.float32)
        for i in range(npol):
            if recs[i, 172] & 1:
                probs[i, [FOUR[1], FOUR[3]]] = 0.9, 0.08
            else:
                probs[i, [FOUR[0], FOUR[2]]] = 0.49
        wins, played, won_at = np.zeros(B, np.int32), np.zeros((B, 2, 81), np.int32), np.zeros((B, 2, 81), np.int32)
        for i in range(B):
            wins[i], played[i], won_at[i] = scripted_record(pos_key(recs[i]))
        values = ((2 * wins - PLAYOUTS) / np.float32(PLAYOUTS)).astype(np.float32)
        return (probs, values, (PLAYOUTS, wins, played, won_at)) if self.records else (probs, values)


class Tree:
    """One manually driven game of a GamePool."""

    def __init__(self, evaluator, rave=None, board=None, **prm):
        prm = dict(dict(rollouts=0, expand_thresh=3), **prm)
        self.pool = selfplay.GamePool([11], selfplay.search_params(**prm), cap=256, threads=1)
        self.lib, self.h = self.pool._lib, self.pool._h
        self.lib.bk_pool_set_manual(self.h, 1)
        if rave is not None:
            self.pool.set_rave(rave)
        self.ev = evaluator
        if board is not None:
            assert self.lib.bk_pool_set_position(self.h, 0, ctypes.byref(go.Game(board)._pos)) == 0
        self.pump()

    def pump(self):
        while True:
            recs, npol = self.pool.collect_positions()
            if len(recs) == 0:
                return
            self.pool.deliver(*self.ev(recs.copy(), npol))

    def rollout(self, n=1):
        self.lib.bk_pool_add_rollouts(self.h, 0, n)
        self.pump()

    def play(self, move):
        assert self.lib.bk_pool_play(self.h, 0, move) == 0
        self.pump()

    def root(self):
        return self.lib.bk_pool_root_id(self.h, 0)

    def node(self, i):
        info, pos = selfplay.NodeInfo(), go.Pos()
        assert self.lib.bk_pool_node(self.h, 0, i, ctypes.byref(info), ctypes.byref(pos)) == 0
        return info, pos_key(np.frombuffer(bytes(pos), np.uint8))

    def children(self, i):
        ids = np.empty(81, np.int32)
        n = self.lib.bk_pool_node_children(self.h, 0, i, ids.ctypes.data, 81)
        return ids[:n].tolist()

    def n_nodes(self):
        return self.pool.info(0)["n_nodes"]

    def visits(self):
        return {self.node(i)[1]: self.node(i)[0].N for i in range(self.n_nodes())}

    def tables(self):
        out = {}
        for i in range(self.n_nodes()):
            t = self.pool.node_rave(0, i)
            if t is not None:
                out[self.node(i)[1]] = (t[0].copy(), t[1].copy())
        return out

    def close(self):
        self.pool.close()


class Model:
    """The backup rule of include/bokego_tree.h in plain Python, keyed by position: it watches one rollout at a time (the
    nodes whose visit count went up are the path), reads nothing of the tree's tables, and keeps its own."""

    def __init__(self, tree):
        self.t, self.N, self.tab = tree, {}, {}
        self.parents = {}                                                 # key -> the keys it was reached from

    def path_of_last_rollout(self):
        t = self.t
        i = t.root()
        info, key = t.node(i)
        path = [(key, info)]
        assert info.N == self.N.get(key, 0) + 1
        while True:
            nxt = [(c,) + t.node(c) for c in t.children(i)]
            nxt = [(c, inf, k) for c, inf, k in nxt if inf.N == self.N.get(k, 0) + 1]
            if not nxt:
                break
            ((i, info, key),) = nxt                                       # exactly one child was visited
            self.parents.setdefault(key, set()).add(path[-1][0])
            path.append((key, info))
        for key, _ in path:
            self.N[key] = self.N.get(key, 0) + 1
        return path

    def rollout(self):
        self.t.rollout(1)
        path = self.path_of_last_rollout()
        L = len(path) - 1
        leaf_key, leaf = path[L]
        if leaf.flags & 2:                                                # a terminal node keeps no record
            return path
        w, played, won_at = scripted_record(leaf_key)
        n = PLAYOUTS
        mv = [info.move for _, info in path]
        for i in range(L + 1):
            if not path[i][1].flags & 8:                                  # no priors: no table
                continue
            rn, rw = self.tab.setdefault(path[i][0], (np.zeros(81, np.int64), np.zeros(81, np.int64)))
            side = (L - i) & 1
            F = set()
            for j in range(i + 1, L + 1):
                m = mv[j]
                if not 0 <= m < 81 or m in F:
                    continue
                F.add(m)
                if (j - i) & 1:
                    rn[m] += n
                    rw[m] += w if side == 0 else n - w
            for s in range(81):
                if s not in F:
                    rn[s] += played[side][s]
                    rw[s] += won_at[side][s]
        return path

    def compare(self):
        got = self.t.tables()
        live = {self.t.node(i)[1] for i in range(self.t.n_nodes())}
        want = {k: v for k, v in self.tab.items() if k in live}          # (a pruning tree has dropped the rest)
        assert set(got) == set(want), (len(got), len(want))
        for k in want:
            assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k[-5:]
            assert (got[k][1] <= got[k][0]).all() and (got[k][1] >= 0).all()
        for k, n in self.t.visits().items():
            assert n == self.N.get(k, 0)
        return len(want)

    def pruned(self):
        """the tree was re-rooted with prune=1: what it dropped starts from nothing if it is ever seen again"""
        live = self.t.visits()
        self.N = {k: v for k, v in self.N.items() if k in live}
        self.tab = {k: v for k, v in self.tab.items() if k in live}


def test_the_tables_equal_a_python_model_of_the_backup_rule():
    t = Tree(Scripted(), rave=16.0, board=NARROW, prune=1)
    m = Model(t)
    assert t.tables() == {}                                               # no recorded rollout yet: no table
    depth = 0
    for _ in range(60):
        depth = max(depth, len(m.rollout()))
    assert m.compare() >= 8 and depth >= 5
    # transpositions: a,b,c,d and c,b,a,d are one node, and rollouts came to it both ways
    assert any(len(p) >= 2 for p in m.parents.values()), "no transposition in the tree"
    root_rn, root_rw = t.pool.node_rave(0, t.root())
    assert root_rn[FOUR[0]] >= PLAYOUTS and root_rn.sum() > 60 * PLAYOUTS
    # after a move the pruning tree keeps the subtree with its tables and records, and goes on from them
    t.play(FOUR[0])
    assert m.compare() >= 3
    m.pruned()
    for _ in range(20):
        m.rollout()
    m.compare()
    # a pass: the new root is reached by one -- a node's children are board points, so the root's own move is the only pass
    # a path can hold, and the rule never reads it -- and the search under it is modelled like any other
    t.play(PASS)
    assert t.node(t.root())[0].move == PASS
    m.compare()
    m.pruned()
    if not t.node(t.root())[0].flags & 2:
        for _ in range(12):
            m.rollout()
    m.compare()
    t.close()


# ---- 4. the selection ---------------------------------------------------------------------------------------------------------------
X, Y = 30, 50


class TwoMoves:
    """Priors 1/2 on X and on Y.  X's playouts (n = 8, four won: value 0) say that the root's side, playing Y first in all
    eight, lost every one; nothing else was ever played."""

    def __call__(self, recs, npol):
        B = len(recs)
        probs = np.zeros((npol, 81), np.float32)
        probs[:, [X, Y]] = 0.5
        wins, played, won_at = np.full(B, 4, np.int32), np.zeros((B, 2, 81), np.int32), np.zeros((B, 2, 81), np.int32)
        played[:, 1, Y] = 8
        return probs, np.zeros(B, np.float32), (8, wins, played, won_at)


def test_the_rave_term_flips_the_choice_on_a_hand_made_node():
    """After the first rollout (X by the tie rule: equal scores, lower point) the plain scores are X: -0 + e / 2 = 0.25 and
    Y: e = 0.5 with e = c_puct * 0.5 * sqrt(1), c_puct = 1: the plain search visits Y.  With RAVE the root's table has
    rn[X] = 8, rw[X] = 4 (tree part: q = 0) and rn[Y] = 8, rw[Y] = 0 (playout part: q = -1); Y is unvisited, so beta = 1 and
    its score is -1 + 0.5 = -0.5 against X's 0 + 0.25: the second rollout goes to X again, by a margin of 0.75."""
    visits = {}
    for k in (16.0, 0.0, None):
        t = Tree(TwoMoves(), rave=k, expand_thresh=100, c_puct=1.0)
        t.rollout(2)
        visits[k] = {mv: n for mv, (n, _) in t.pool.root_children(0).items() if n}
        if k:
            rn, rw = t.pool.node_rave(0, t.root())
            assert (rn[X], rw[X], rn[Y], rw[Y]) == (16, 8, 16, 0) and rn.sum() == 32 and rw.sum() == 8
        else:
            assert t.pool.node_rave(0, t.root()) is None
        t.close()
    assert visits[16.0] == {X: 2} and visits[0.0] == visits[None] == {X: 1, Y: 1}


# ---- 5. searches that must equal RAVE off ----------------------------------------------------------------------------------------
def searched(tree, n=60):
    tree.rollout(n)
    out = (tree.pool.root_children(0), sorted(tree.visits().items()), tree.pool.info(0))
    return out


def test_without_records_or_with_equiv_0_the_search_is_the_plain_one():
    plain = Tree(Scripted(records=False))
    want = searched(plain)
    for ev, k in ((Scripted(records=False), 16.0),                        # RAVE on, but the records are never delivered
                  (Scripted(), 0.0),                                      # records delivered, RAVE off
                  (Scripted(), None)):                                    # ... to a pool that never heard of RAVE
        t = Tree(ev, rave=k)
        assert searched(t) == want and t.tables() == {}
        if not k:
            assert t.pool.snapshot(0) == plain.pool.snapshot(0)          # off: the bytes of a pool that never heard of RAVE
        t.close()
    on = Tree(Scripted(), rave=16.0)
    assert searched(on)[0] != want[0] and len(on.tables()) > 0             # (the records do enter the search)
    on.pool.set_rave(0)                                                   # switched off: tables and records go
    assert on.tables() == {}
    on.close()
    plain.close()


# ---- 6. what bk_pool_set_rave refuses ------------------------------------------------------------------------------------------------
def test_set_rave_refuses_what_it_cannot_do():
    lib = selfplay.treelib()

    def pool(**prm):
        return selfplay.GamePool([1], selfplay.search_params(rollouts=0, **prm), cap=128, threads=1)

    p = pool()
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), float("-inf")):
        assert lib.bk_pool_set_rave(p._h, bad) == -1
        with pytest.raises(ValueError):
            p.set_rave(bad)
    assert lib.bk_pool_set_rave(p._h, 16.0) == 0 and lib.bk_pool_set_rave(p._h, 0.0) == 0
    p.close()
    for prm in (dict(leaves=4), dict(simulate=1, value_weight=1.0), dict(use_value=0), dict(value_weight=0.5)):
        p = pool(**prm)
        assert lib.bk_pool_set_rave(p._h, 16.0) == -1, prm
        before = p.snapshot(0)
        with pytest.raises(ValueError):
            p.set_rave(16.0)
        assert p.snapshot(0) == before                                    # nothing changed
        p.close()
    rn = np.empty(81, np.int64)
    p = pool()
    assert lib.bk_pool_node_rave(p._h, 0, 0, rn.ctypes.data, rn.ctypes.data) == -1
    assert lib.bk_pool_node_rave(p._h, 3, 0, rn.ctypes.data, rn.ctypes.data) == -1
    p.close()


# ---- 7. snapshots ---------------------------------------------------------------------------------------------------------------------
def test_a_restored_game_continues_rollout_for_rollout():
    a = Tree(Scripted(), rave=16.0, prune=1)
    a.rollout(30)
    blob = a.pool.snapshot(0)
    b = Tree(Scripted())                                                  # any pool: parameters and RAVE come with the snapshot
    b.pool.restore(0, blob)
    assert b.pool.snapshot(0) == blob
    for t in (a, b):
        t.rollout(20)
        t.play(FOUR[0])
        t.rollout(10)
    assert a.pool.root_children(0) == b.pool.root_children(0) and a.visits() == b.visits()
    ta, tb = a.tables(), b.tables()
    assert set(ta) == set(tb) and len(ta) > 0
    assert all(np.array_equal(ta[k][0], tb[k][0]) and np.array_equal(ta[k][1], tb[k][1]) for k in ta)
    assert a.pool.snapshot(0) == b.pool.snapshot(0)
    # a snapshot whose tables are damaged is refused and the game stays as it was
    bad = bytearray(a.pool.snapshot(0))
    bad[-4:] = b"\xff\xff\xff\x7f"                                        # the last won_at count: beyond its played count
    with pytest.raises(ValueError):
        b.pool.restore(0, bytes(bad))
    with pytest.raises(ValueError):
        b.pool.restore(0, a.pool.snapshot(0)[:-8])
    assert a.pool.snapshot(0) == b.pool.snapshot(0)
    a.close()
    b.close()


# ---- 8. the evaluator and the whole search on the host ------------------------------------------------------------------------
def records_of(games):
    return np.stack([np.frombuffer(bytes(g._pos), np.uint8) for g in games])


def test_playout_amaf_and_the_evaluator_with_both_sides():
    passed = go.Game()
    passed.play_move(40)
    passed.play_pass()
    recs = records_of([go.Game(BOARD), go.Game(), passed])
    n = 3
    one = RO.playout_amaf(recs, n, 3, rules="host")
    two = RO.playout_amaf(recs, n, 3, rules="host", sides=2)
    assert two.played.shape == two.won.shape == (3, 2, 81) and two.played.dtype == two.won.dtype == np.int32
    assert np.array_equal(two.value.view(np.int32), one.value.view(np.int32)) and np.array_equal(two.wins, one.wins)
    assert np.array_equal(two.played[:, 0], one.played) and np.array_equal(two.won[:, 0], one.won)
    assert (two.played.sum(1) <= n).all() and (two.won <= two.played).all()
    assert (two.won[:, 0].max(1) <= two.wins).all() and (two.won[:, 1].max(1) <= n - two.wins).all()
    assert two.played[1, 1].sum() > n * 15                                # the empty board: the opponent plays too
    assert not two.played[0, 1].any()                                     # every playout of BOARD is [38, pass, pass]
    assert np.array_equal(RO.amaf_prior(recs, two), RO.amaf_prior(recs, one))
    with pytest.raises(ValueError):
        RO.playout_amaf(recs, n, 3, rules="host", sides=3)
    # the evaluator: probs and values as without rave, and the records of ALL rows
    ev = RO.PlayoutEvaluator(None, n, seed=3, rules="host", prior=1.0, rave=True)
    probs, values, records = ev(recs, 2)
    p0, v0 = RO.PlayoutEvaluator(None, n, seed=3, rules="host", prior=1.0)(recs, 2)
    assert np.array_equal(probs, p0) and np.array_equal(values, v0)
    playouts, wins, played, won_at = records
    assert playouts == n and np.array_equal(wins, two.wins) and wins.dtype == played.dtype == won_at.dtype == np.int32
    assert np.array_equal(played, two.played) and np.array_equal(won_at, two.won)
    probs, values, records = ev(recs, 0)                                  # no policy row: records all the same
    assert probs.shape == (0, 81) and np.array_equal(records[2], two.played)
    assert len(RO.PlayoutEvaluator(None, n, seed=3, rules="host", prior=1.0)(recs, 0)) == 2


def test_native_mcts_with_rave_on_the_host_rules():
    t = NativeMCTS(Position(board=BOARD), None, None, playout_value=7, playout_prior=1.0, playout_rave=16,
                   playout_rules="host", expand_thresh=1)
    assert t.playout_rave == 16.0 and t.evaluator.rave and t.evaluator.prior == 1.0
    assert t.rave() is None
    t.rollout(6)
    rn, rw = t.rave()
    assert rn.dtype == rw.dtype == np.int64 and rn[38] >= 7 and rn[38] == rw[38] and t.rave(t.root) is not None
    assert t.rave(Position()) is None                                     # a position the tree never saw
    for other in (copy.deepcopy(t), pickle.loads(pickle.dumps(t))):
        assert np.array_equal(other.rave()[0], rn) and np.array_equal(other.rave()[1], rw) and other.playout_rave == 16.0
        other.rollout(2)                                                  # (the unpickled tree rebuilds its evaluator: rave again)
        assert other.evaluator.rave and other.rave()[0].sum() > rn.sum()
        other.close()
    assert t.choose().last_move == 38
    t.close()
    t = NativeMCTS(Position(), None, None, playout_value=2, playout_prior=1.0, playout_rave=4, playout_rules="host",
                   expand_thresh=1, playout_patterns=np.full(131072, 300, np.uint16), playout_tactics=np.full(64, 256, np.uint16))
    t.rollout(3)
    assert t.rave()[0].sum() > 0 and t.evaluator.patterns is not None and t.evaluator.tactics is not None
    t.close()
    plain = NativeMCTS(Position(board=BOARD), None, None, playout_value=2, playout_prior=1.0, playout_rules="host")
    assert plain.playout_rave == 0.0 and not plain.evaluator.rave and plain.rave() is None
    plain.close()
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(Position(), None, None, playout_rave=16)
    with pytest.raises(TypeError, match="playout_value"):
        NativeMCTS(Position(), lambda x: x, lambda x: x, playout_rave=16)
    for bad in (-1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            NativeMCTS(Position(), None, None, playout_value=2, playout_prior=1.0, playout_rave=bad, playout_rules="host")


def test_command_lines(capsys):
    assert gtp.parse_args([]).playout_rave == 0.0
    a = gtp.parse_args(["--playout-value", "64", "--playout-prior", "1", "--playout-rave", "4", "-r", "400"])
    assert (a.playout_value, a.playout_prior, a.playout_rave, a.r) == (64, 1.0, 4.0, 400)
    assert gtp.parse_args(["--playout-value", "64", "--playout-rave"]).playout_rave == 4.0      # the shipped default
    for bad in (["--playout-rave", "16"], ["--playout-rave"], ["--playout-value", "8", "--playout-rave", "-1"],
                ["--playout-value", "8", "--playout-rave", "inf"], ["--playout-value", "8", "--playout-rave", "x"]):
        with pytest.raises(SystemExit):
            gtp.parse_args(bad)
    assert match.parse_args([]).playout_rave == 0.0
    a = match.parse_args(["--playout-value", "64", "--playout-prior", "1", "--playout-rave", "64", "--games", "100"])
    assert (a.playout_value, a.playout_rave, a.games) == (64, 64.0, 100)
    assert match.parse_args(["--playout-value", "64", "--playout-rave"]).playout_rave == 4.0
    for bad in (["--playout-rave", "16"], ["--playout-value", "8", "--playout-rave", "nan"],
                ["--playout-value", "8", "--playout-rave", "16", "--engine", "python -m oracle.gtp_cpu"]):
        with pytest.raises(SystemExit):
            match.parse_args(bad)
    a = RO._parse(["--sgf", "g.sgf", "--random", "--amaf", "--sides", "2"])
    assert a.sides == 2 and RO._parse(["--sgf", "g.sgf", "--random", "--amaf"]).sides == 1
    for bad in (["--sgf", "g.sgf", "--random", "--sides", "2"], ["--sgf", "g.sgf", "--random", "--amaf", "--sides", "3"]):
        with pytest.raises(SystemExit):
            RO._parse(bad)
    capsys.readouterr()

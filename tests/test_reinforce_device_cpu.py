"""CPU: what the device-resident REINFORCE playouts add that needs no GPU -- the bkt_area_score symbol and declaration, the
new arguments of reinforce.play_games, the resources of bk_playout.hip's kernels, and a numpy mirror of the area score and
owner map (the one tests/test_gpu_reinforce_device.py compares the kernel's owner map with) against bk_pos_area_score."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from bokego_amd import _trainlib as T
from bokego_amd import go
from bokego_amd import reinforce as R
from conftest import REPO

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"
KOMI = 5.5


# ---- the numpy mirror: a plain flood fill ---------------------------------------------------------------------------------
def area_mirror(board):
    """board: 81 values 0 empty / 1 black / 2 white -> (black area, white area, owner int8 [81]: +1 / -1 / 0)."""
    board = np.asarray(board).reshape(81)
    owner = np.where(board == 1, 1, np.where(board == 2, -1, 0)).astype(np.int8)
    seen = board != 0
    for s in range(81):
        if seen[s]:
            continue
        region, stack, touch = [], [s], set()
        seen[s] = True
        while stack:
            q = stack.pop()
            region.append(q)
            r, c = divmod(q, 9)
            for rr, cc in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)):
                if not (0 <= rr < 9 and 0 <= cc < 9):
                    continue
                t = 9 * rr + cc
                if board[t]:
                    touch.add(int(board[t]))
                elif not seen[t]:
                    seen[t] = True
                    stack.append(t)
        if touch == {1}:
            owner[region] = 1
        elif touch == {2}:
            owner[region] = -1
    return int((owner == 1).sum()), int((owner == -1).sum()), owner


def mirror_score(board, komi=KOMI):
    """-> (the host's float: (float)black - ((float)white + komi) in float32, owner)."""
    b, w, owner = area_mirror(board)
    return np.float32(b) - (np.float32(w) + np.float32(komi)), owner


def records_from_boards(boards):
    """bk_pos records uint8 [n, 192] with the given boards ([n, 81] of 0 / 1 / 2), black to move: the area score reads the
    board only."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 81)
    recs = R.initial_positions(len(boards))
    recs[:, :81] = boards
    return recs


def host_scores(recs, komi=KOMI):
    lib = go.golib()
    recs = np.ascontiguousarray(recs)
    return np.array([lib.bk_pos_area_score(ctypes.cast(recs[i].ctypes.data, ctypes.POINTER(go.Pos)), komi)
                     for i in range(len(recs))], np.float32)


def random_boards(n, seed):
    """n boards whose stone density runs from nearly empty to nearly full, the two colours in varied proportion."""
    rng = np.random.default_rng(seed)
    density = rng.random(n)[:, None]
    black_share = rng.random(n)[:, None]
    u, v = rng.random((n, 81)), rng.random((n, 81))
    return np.where(u < density, np.where(v < black_share, 1, 2), 0).astype(np.uint8)


def _board(text):
    return np.array([".XO".index(ch) for ch in text.replace(" ", "").replace("\n", "")], np.uint8)


def crafted_boards():
    """name -> (board, expected score or None)."""
    eyes = np.full(81, 2, np.uint8)
    eyes[[0, 80]] = 0                                    # white everywhere but two one-point eyes
    both = _board(". . . X . O . . ." * 9)               # columns 0-2 black's, 6-8 white's, column 4 touches both
    edge = _board(". . . X . . . . ." * 9)               # one colour and the edge: every empty point is black's
    mixed = _board("""
        . X . . . . O . .
        X X . . . . O O O
        . . . . . . . . .
        . . X X X . . . .
        . . X . X . . O .
        . . X X X . O . O
        . . . . . . . O .
        O O . . . . . . .
        . O . . . . . X .""")
    return {"empty": (np.zeros(81, np.uint8), -5.5), "two_eyes": (eyes, -86.5), "both_colours": (both, None),
            "edge_and_black": (edge, 81 - 5.5), "mixed": (mixed, None)}


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_area_score_is_bound_and_declared():
    assert "bkt_area_score" in T.SYMBOLS
    assert T.BKT_ABI_VERSION == 4
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bkt_area_score\s*\(\s*const\s+void\s*\*\s*pos\s*,\s*int\s+batch\s*,\s*float\s+komi\s*,"
                     r"\s*float\s*\*\s*score\s*,\s*int8_t\s*\*\s*owner\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"#define\s+BKT_ABI_VERSION\s+4\b", src)
    assert callable(T.area_score)


# ---- play_games' new arguments -------------------------------------------------------------------------------------------
def test_play_games_takes_rules_and_start():
    p = inspect.signature(R.play_games).parameters
    assert p["rules"].default == "device" and p["start"].default is None


def test_unknown_rules_are_refused_before_the_gpu_is_touched():
    with pytest.raises(ValueError, match="rules"):
        R.play_games(None, None, 2, 2, seed=1, rules="gpu")          # no engines, no GPU: the check comes first


@pytest.mark.parametrize("rules", ["device", "host"])
def test_start_must_have_black_to_move(rules):
    g = go.Game()
    g.play_move(40)
    start = R.initial_positions(4)
    start[2] = np.frombuffer(bytes(g._pos), np.uint8)                # turn 1
    with pytest.raises(ValueError, match="turn"):
        R.play_games(None, None, 2, 2, seed=1, rules=rules, start=start)
    with pytest.raises(ValueError, match="start"):
        R.play_games(None, None, 2, 2, seed=1, rules=rules, start=R.initial_positions(3))


# ---- the kernels' resources ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_playout_kernels_build_without_spills_or_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_playout.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert any("area_score_kernel" in k for k in kernels), kernels
    assert any("play_moves_kernel" in k for k in kernels), kernels
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(spills) == 2 * len(kernels) and len(scratch) == len(kernels)
    assert all(int(n) == 0 for _, n in spills), spills
    assert all(int(n) == 0 for n in scratch), scratch


# ---- the mirror against the host rules -----------------------------------------------------------------------------------
def test_mirror_equals_the_host_on_random_boards():
    boards = random_boards(3000, 20)
    got = np.array([mirror_score(b)[0] for b in boards], np.float32)
    want = host_scores(records_from_boards(boards))
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.nonzero(got != want)[0][:10]
    assert len(np.unique(want)) > 100                                # the boards do vary


def test_mirror_equals_the_host_on_other_komi():
    boards = random_boards(200, 21)
    for komi in (0.0, 6.5, 7.0, -0.5):
        got = np.array([mirror_score(b, komi)[0] for b in boards], np.float32)
        assert np.array_equal(got, host_scores(records_from_boards(boards), komi)), komi


def test_crafted_boards():
    for name, (board, score) in crafted_boards().items():
        got, owner = mirror_score(board)
        assert got == host_scores(records_from_boards(board[None]))[0], name
        if score is not None:
            assert got == np.float32(score), name
        assert np.array_equal(owner[board == 1], np.ones((board == 1).sum())), name
        assert np.array_equal(owner[board == 2], -np.ones((board == 2).sum())), name
    c = crafted_boards()
    assert not mirror_score(c["empty"][0])[1].any()
    assert (mirror_score(c["two_eyes"][0])[1] == -1).all()
    own = mirror_score(c["both_colours"][0])[1].reshape(9, 9)
    assert (own[:, :4] == 1).all() and (own[:, 4] == 0).all() and (own[:, 5:] == -1).all()
    assert (mirror_score(c["edge_and_black"][0])[1] == 1).all()
    mixed = mirror_score(c["mixed"][0])[1].reshape(9, 9)
    assert mixed[0, 0] == 1 and mixed[4, 3] == 1 and mixed[8, 0] == -1 and mixed[5, 7] == -1 and mixed[2, 4] == 0

"""-m "not gpu": the value-data generator's file format, its counter layouts and their numpy mirror, the value-row dataset
of train --values, and the command-line checks (bokego_amd/genvals.py, bokego_amd/train.py)."""
import ctypes
import os

import numpy as np
import pytest

from bokego_amd import genvals as GV
from bokego_amd import go, train
from bokego_amd import reinforce as R
from conftest import GOLDEN


def _random_rows(n, seed):
    """n rows from host games of random legal moves, labelled alternately."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        g = go.Game()
        for _ in range(int(rng.integers(5, 60))):
            legal = [m for m in range(81) if g.is_legal(m)]
            if not legal:
                break
            g.play_move(int(rng.choice(legal)))
        rows.append((g.board, -1 if g.ko is None else g.ko, g.last_move, g.turn, 1 if i % 2 else -1))
    return rows


# ---- the CSV --------------------------------------------------------------------------------------------------------------
def test_csv_header_append_and_roundtrip(tmp_path):
    p = str(tmp_path / "v.csv")
    rows = _random_rows(6, 1)
    GV.write_rows(p, rows[:4])
    GV.write_rows(p, rows[4:])
    with open(p) as f:
        lines = f.read().splitlines()
    assert lines[0] == "board,ko,last,turn,val" and lines.count(lines[0]) == 1
    assert len(lines) == 7
    assert GV.read_rows(p) == [tuple(r) for r in rows]


def test_csv_header_written_into_an_empty_file(tmp_path):
    p = tmp_path / "v.csv"
    p.write_text("")
    GV.write_rows(str(p), _random_rows(1, 2))
    assert p.read_text().splitlines()[0] == GV.HEADER


def test_csv_foreign_header_refused(tmp_path):
    p = tmp_path / "v.csv"
    p.write_text("board,last,ko,val\n" + "." * 81 + ",-1,3,1\n")
    before = p.read_text()
    with pytest.raises(ValueError):
        GV.write_rows(str(p), _random_rows(1, 3))
    with pytest.raises(ValueError):
        GV.read_rows(str(p))
    assert p.read_text() == before


# ---- counters --------------------------------------------------------------------------------------------------------------
def test_move_counter_layout():
    ids = np.array([0, 1, 4095, 2 ** 32 + 7], np.int64)
    c = GV.move_counters(ids, 37).view(np.uint32)
    assert c.tolist() == [[0, 37, 0, 0], [1, 37, 0, 0], [4095, 37, 0, 0], [7, 37, 1, 0]]


def test_random_ply_mirror_and_range():
    ids = np.arange(20000, dtype=np.int64)
    r = GV.random_ply(ids, 12345)
    assert r.min() >= 70 and r.max() < 90
    assert set(r.tolist()) == set(range(70, 90))
    counts = np.bincount(r - 70, minlength=20)
    assert counts.min() > 800 and counts.max() < 1200
    # the documented counter (g mod 2^32, 0, g >> 32, 1) through the Philox mirror
    c = np.zeros((len(ids), 4), np.uint32)
    c[:, 0], c[:, 3] = ids, 1
    u = R.uniform(R.philox4x32_10(c, R.seed_key(12345))[:, 0])
    assert np.array_equal(r, 70 + np.floor(u * 20).astype(np.int64))
    # a game's draw depends on its id only: any subset, in any order, draws the same
    sub = np.array([19999, 3, 512, 4096])
    assert np.array_equal(GV.random_ply(sub, 12345), r[sub])
    assert not np.array_equal(GV.random_ply(ids, 12346), r)


# ---- train --values -------------------------------------------------------------------------------------------------------
def test_value_record_dataset_planes_and_targets(tmp_path):
    p = str(tmp_path / "v.csv")
    rows = _random_rows(12, 4)
    GV.write_rows(p, rows)
    ds = train.ValueRecordDataset([p])
    assert len(ds) == 12
    lib = go.golib()
    for i, (board, ko, last, turn, val) in enumerate(rows):
        pos = go.Pos()
        assert lib.bk_pos_from_board(ctypes.byref(pos), board.encode(), ko, last, turn) == 0
        want = np.empty((27, 9, 9), np.uint8)
        lib.bk_pos_features_u8(ctypes.byref(pos), want.ctypes.data, 1)
        assert np.array_equal(ds.planes[i], want)
    assert ds.value.tolist() == [float(r[4]) for r in rows]
    assert set(ds.value.tolist()) == {1.0, -1.0}
    assert not ds.has_policy.any() and not ds.policy.any()


def test_merge_keeps_record_rows_first(tmp_path):
    p = str(tmp_path / "v.csv")
    GV.write_rows(p, _random_rows(3, 5))
    a = train.ValueRecordDataset([p])
    m = train.merge_datasets(a, train.ValueRecordDataset([p], seed=9))
    assert len(m) == 6 and m.seed == a.seed
    assert np.array_equal(m.planes[:3], a.planes) and np.array_equal(m.planes[3:], a.planes)


def test_value_row_with_bad_label_refused(tmp_path):
    p = tmp_path / "v.csv"
    p.write_text(GV.HEADER + "\n" + "." * 81 + ",-1,40,1,0\n")
    with pytest.raises(ValueError):
        train.ValueRecordDataset([str(p)])


# ---- command-line checks ---------------------------------------------------------------------------------------------------
def _pool(tmp_path):
    import shutil
    d = tmp_path / "pool"
    d.mkdir()
    for i in (0, 3, 7):
        shutil.copy(os.path.join(GOLDEN, "policy_19.bkw"), d / f"policy_{i}.bkw")
    return d


@pytest.mark.parametrize("argv", [
    ["-o", "x.csv"],                                     # no policies
    ["-o", "x.csv", "--sl", "a.pt"],                     # --rl missing
    ["-o", "x.csv", "-w", ".", "--sl", "a.pt"],          # both forms
    ["-o", "x.csv", "--sl", "a.pt", "--rl", "b.pt", "--batch", "0"],
    ["-o", "x.csv", "--sl", "a.pt", "--rl", "b.pt", "--batch", "65537"],
    ["-o", "x.csv", "--sl", "a.pt", "--rl", "b.pt", "--games", "0"],
])
def test_genvals_argument_errors(argv):
    with pytest.raises(SystemExit) as e:
        GV._parse(argv)
    assert e.value.code == 2


def test_genvals_pool_and_counts(tmp_path):
    d = _pool(tmp_path)
    a = GV._parse(["-o", "x.csv", "-w", str(d), "-n", "3", "--batch", "65536"])
    assert a.sl.endswith("policy_0.bkw") and a.rl.endswith("policy_7.bkw")
    assert a.games == 3000 and a.batch == 65536
    assert GV._parse(["-o", "x.csv", "-w", str(d), "--games", "17"]).games == 17
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(SystemExit):
        GV._parse(["-o", "x.csv", "-w", str(empty)])


@pytest.mark.parametrize("argv", [
    ["--values", "v.csv", "--net", "policy"],
    ["--values", "v.csv"],                               # --net both: no policy targets
    ["--net", "value"],                                  # neither --records nor --values
])
def test_train_values_argument_errors(argv):
    with pytest.raises(SystemExit) as e:
        train.main(argv)
    assert e.value.code == 2

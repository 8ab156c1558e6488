"""Training without a GPU: self-play records -> RecordDataset, the dihedral symmetries, checkpoint names, and the
shape of libbktrain.so (exports, no register spills)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from bokego_amd import go, nnet, selfplay
from bokego_amd import train
from bokego_amd.bkw import load_bkw
from conftest import GOLDEN, REPO

CSRC = os.path.join(REPO, "bokego_amd", "csrc")
TRAIN_LIB = os.path.join(REPO, "bokego_amd", "libbktrain.so")
HEADER = os.path.join(REPO, "include", "bokego_train.h")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """a 3-game self-play on the oracle nets with the root visit counts recorded, as selfplay --out writes it"""
    from oracle.oracle import OraclePolicy, OracleValue
    pol = OraclePolicy(load_bkw(os.path.join(GOLDEN, "policy_19.bkw")))
    val = OracleValue(load_bkw(os.path.join(GOLDEN, "value_synth.bkw")))
    ev = selfplay.CallableEvaluator(lambda x: pol(x), lambda x: val(x))
    local, _ = selfplay.self_play(ev, n_games=3, rollouts=20, expand_thresh=4, max_turns=12, cap=400, threads=1,
                                  record_visits=1)
    d = tmp_path_factory.mktemp("records")
    selfplay.write_records(str(d / "rank0"), local["games"], local["visits"])
    return d, local


def test_record_dataset_one_position_per_ply(records):
    d, local = records
    ds = train.RecordDataset([str(d)])
    games = local["games"]
    assert len(ds) == sum(len(g["moves"]) for g in games.values())
    assert ds.planes.dtype == np.uint8 and ds.planes.shape == (len(ds), 27, 9, 9)
    i = 0
    for gid in sorted(games):
        g = go.Game()
        for ply, mv in enumerate(games[gid]["moves"]):
            assert ds.game_of[i] == (0, gid, ply)
            # the incremental planes the search saw (the liberty cache carried along), not fresh ones
            assert np.array_equal(ds.planes[i], g.features_u8())
            assert ds.has_policy[i] == (mv != go.PASS)
            g.play_move(mv)
            i += 1


def test_record_dataset_policy_targets_are_the_visit_counts(records):
    d, local = records
    ds = train.RecordDataset([str(d)])
    i = 0
    for gid in sorted(local["games"]):
        for ply, mv in enumerate(local["games"][gid]["moves"]):
            p = ds.policy[i]
            if mv == go.PASS:
                assert not p.any()
            else:
                vis = {k: n for k, n in local["visits"][gid][ply].items() if n > 0}
                assert abs(p.sum() - 1) < 1e-6
                assert set(np.flatnonzero(p).tolist()) == set(vis)
                tot = sum(vis.values())
                for k, n in vis.items():
                    assert abs(p[k] - n / tot) < 1e-6
            i += 1


def test_record_dataset_value_targets_follow_the_side_to_move(records):
    d, local = records
    ds = train.RecordDataset([str(d)])
    i = 0
    for gid in sorted(local["games"]):
        g = local["games"][gid]
        black_won = g["score"] > 0
        prev = None
        for ply in range(len(g["moves"])):
            z = ds.value[i]
            assert z in (1.0, -1.0)
            if prev is not None:
                assert z == -prev          # one ply later the other side is to move
            # plane 3 of the planes the value head sees is all ones when black is to move (nnet.py:182-262):
            # +1 means the side to move won
            black_to_move = bool(ds.planes[i][3].all())
            assert black_to_move == (ply % 2 == 0)
            assert (z > 0) == (black_to_move == black_won)
            prev, i = z, i + 1


def test_record_dataset_without_visits_uses_the_played_move(tmp_path):
    moves = [40, 41, go.PASS, 30]
    selfplay.write_records(str(tmp_path), {0: {"moves": moves, "score": -3.5}})
    ds = train.RecordDataset(str(tmp_path))
    assert len(ds) == 4 and ds.has_policy.tolist() == [True, True, False, True]
    for i, mv in enumerate(moves):
        if mv != go.PASS:
            assert ds.policy[i].argmax() == mv and ds.policy[i].sum() == 1
    assert ds.value.tolist() == [-1, 1, -1, 1]   # white won: black (to move at plies 0, 2) loses


def test_dihedral_maps_form_a_group():
    P = train.DIHEDRAL
    ident = np.arange(81)
    assert len({tuple(p) for p in P}) == 8
    assert any(np.array_equal(p, ident) for p in P)
    perms = {tuple(p) for p in P}
    for g in range(8):
        assert np.array_equal(P[g][train.DIHEDRAL_INVERSE[g]], ident)
        assert np.array_equal(train.DIHEDRAL_INVERSE[g][P[g]], ident)
        for h in range(8):
            assert tuple(P[g][P[h]]) in perms   # closed under composition


def test_targets_move_with_their_planes():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 5, (4, 27, 9, 9)).astype(np.uint8)
    pol = np.zeros((4, 81), np.float32)
    for b in range(4):
        pol[b, 9 * b + 2] = 1
    for g in range(8):
        xt, pt = train.apply_symmetry(x, g), train.apply_symmetry(pol, g)
        for b in range(4):
            q = int(pol[b].argmax())
            d = int(pt[b].argmax())
            # the point the target moved to carries the planes of the point it came from
            assert np.array_equal(xt[b].reshape(27, 81)[:, d], x[b].reshape(27, 81)[:, q])
        ginv = int(np.flatnonzero([np.array_equal(train.DIHEDRAL[k], train.DIHEDRAL_INVERSE[g]) for k in range(8)])[0])
        assert np.array_equal(train.apply_symmetry(xt, ginv), x)


def test_symmetric_boards_give_symmetric_planes():
    """features of the transformed board (built fresh from its board string) == the transformed features"""
    rng = np.random.default_rng(11)
    for trial in range(6):
        g = go.Game()
        for _ in range(int(rng.integers(10, 40))):
            legal = g.get_legal_moves()
            if not legal:
                break
            g.play_move(int(rng.choice(legal)))
        board = g.board
        fresh = go.Game(board=board, turn=g.turn).features_u8(fresh=True)
        for s in range(8):
            perm = train.DIHEDRAL[s]
            tb = "".join(board[perm[q]] for q in range(81))
            ft = go.Game(board=tb, turn=g.turn).features_u8(fresh=True)
            assert np.array_equal(ft, train.apply_symmetry(fresh, s)), (trial, s)


def test_augmented_batches_are_seeded_and_consistent(records):
    d, _ = records
    ds = train.RecordDataset([str(d)], augment=True, seed=4)
    a = [[t.clone() for t in b] for b in ds.batches(8, epoch=1, device="cpu")]
    b = [[t.clone() for t in b] for b in ds.batches(8, epoch=1, device="cpu")]
    assert len(a) == len(b) and all(torch.equal(u, v) for x, y in zip(a, b) for u, v in zip(x, y))
    plain = list(train.RecordDataset([str(d)], seed=4).batches(8, epoch=1, device="cpu"))
    for (xa, pa, ha, va), (xp, pp, hp, vp) in zip(a, plain):
        assert torch.equal(ha, hp) and torch.equal(va, vp)
        for r in range(len(xa)):
            hits = [s for s in range(8)
                    if np.array_equal(train.apply_symmetry(xp[r].numpy(), s), xa[r].numpy())
                    and np.array_equal(train.apply_symmetry(pp[r].numpy(), s), pa[r].numpy())]
            assert hits


def test_checkpoint_keys_are_the_reference_names():
    counters = [f"conv.{b}.num_batches_tracked" for b in (1, 4, 7, 10, 13, 16, 19)]
    p = train.TrainablePolicyNet(device="cpu")
    assert set(p.state_dict()) == set(nnet._TRUNK_NAMES) | set(counters)
    v = train.TrainableValueNet(device="cpu")
    assert set(v.state_dict()) == set(nnet._VALUE_NAMES) | set(counters) | {"bn.num_batches_tracked",
                                                                             "lin_bn.num_batches_tracked"}
    # a BKW file loads with the shapes the reference uses, and HipPolicyNet takes the state_dict back
    sd = train.load_weights(os.path.join(GOLDEN, "value_synth.bkw"))
    v2 = train.TrainableValueNet.from_state_dict(sd, device="cpu")
    got = v2.state_dict()
    for k, a in load_bkw(os.path.join(GOLDEN, "value_synth.bkw")).items():
        assert np.array_equal(got[k].numpy(), a), k
    hp = nnet.HipValueNet(got)
    assert set(hp.state_dict()) == set(got)


def test_cli_refuses_a_batch_of_one(records, capsys):
    d, _ = records
    with pytest.raises(SystemExit):
        train.main(["--records", str(d), "-b", "1"])
    assert "BatchNorm" in capsys.readouterr().err


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(bkt_\w+)\s*\(", src))


def test_library_exports_exactly_the_header():
    if not os.path.exists(TRAIN_LIB):
        subprocess.check_call(["make", "-C", CSRC, "../libbktrain.so"])
    out = subprocess.run(["nm", "-D", "--defined-only", TRAIN_LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-2] in ("T", "W")}
    ours = {s for s in exported if s.startswith("bkt_")}
    assert ours == _declared()
    assert not {s for s in exported if not s.startswith("bkt_") and not s.startswith("_")} - {"main"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_kernels_build_without_spills(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "bk_train.hip"),
                        "-o", str(tmp_path / "t.so")], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    spills = re.findall(r"(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(kernels) >= 10 and len(spills) == 2 * len(kernels)
    assert all(int(n) == 0 for _, n in spills)

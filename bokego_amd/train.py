"""Training of the reference's PolicyNet / ValueNet on the MI355X from self-play records.

    python -m bokego_amd.train --records r/ --net policy|value|both [-c CKPT [CKPT]] [--init-trunk-from policy.pt]
                               -e EPOCHS -b BATCH --lr LR --seed S --out DIR [--precision fp32|bf16]
    python -m bokego_amd.train --values values.csv [...] --net value [--records r/] ...

closes the loop `selfplay --out r/` -> `train --records r/` -> `selfplay --policy out/policy_1.pt`, and
`genvals -o values.csv` -> `train --values values.csv --net value` -> `selfplay --value out/value_1.pt`.

The trunk (seven conv -> BatchNorm2d -> ReLU blocks) runs on the HIP kernels of libbktrain.so (bokego_amd/_trainlib.py),
one torch.autograd.Function per block (train-mode BatchNorm; in eval mode with gradients enabled, BatchNorm with its
running statistics frozen, as REINFORCE needs); torch's own convolution never runs on it.  The heads -- the untied-bias 1x1
conv.21 (a sum over channels here), the value net's bn / lin1 / lin_bn / lin2 / tanh -- the losses and Adam are torch
ops on the device, about 0.02 % of the FLOPs.  Parameter and buffer names are the reference's state_dict names
(bokego/nnet.py:31-57, 73-113), so state_dict() is a reference checkpoint: HipPolicyNet.load_state_dict,
bkw.convert_pt, `selfplay --policy` and `gtp -p` take it as it is.
"""
import argparse
import json
import math
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import _trainlib as T
from . import go
from .engine import _BN, _CONV

N_TRUNK = len(_CONV)


# ---- the networks -------------------------------------------------------------------------------------------------
class _TrunkBlock(torch.autograd.Function):
    """conv (k = 5 or 3, pad k//2) -> train-mode BatchNorm2d -> ReLU; updates the BN running buffers in place."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                precision="fp32"):
        x = x.contiguous()
        z = T.conv_forward(x, w.detach().contiguous(), b.detach().contiguous(), precision=precision)
        y, mean, invstd = T.bn_relu_train(z, gamma.detach().contiguous(), beta.detach().contiguous(), running_mean,
                                          running_var, num_batches_tracked, momentum, eps)
        ctx.save_for_backward(x, w, z, y, gamma, mean, invstd)
        ctx.precision = precision
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, z, y, gamma, mean, invstd = ctx.saved_tensors
        dz, dgamma, dbeta = T.bn_relu_backward(dy.contiguous(), y, z, gamma.detach().contiguous(), mean, invstd)
        dw, db = T.conv_wgrad(x, dz, w.shape, precision=ctx.precision)
        dx = (T.conv_dgrad(dz, w.detach().contiguous(), precision=ctx.precision) if ctx.needs_input_grad[0]
              else None)
        return dx, dw, db, dgamma, dbeta, None, None, None, None, None, None


class _TrunkBlockEval(torch.autograd.Function):
    """conv (k = 5 or 3, pad k//2) -> eval-mode BatchNorm2d (running statistics, left unchanged) -> ReLU, with the
    gradient of that function: the same kernels and bits forward as the no-grad eval path."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, running_mean, running_var, eps, precision="fp32"):
        x = x.contiguous()
        z = T.conv_forward(x, w.detach().contiguous(), b.detach().contiguous(), precision=precision)
        y = T.bn_relu_eval(z, gamma.detach().contiguous(), beta.detach().contiguous(), running_mean, running_var, eps)
        ctx.save_for_backward(x, w, z, y, gamma, running_mean, running_var)
        ctx.eps = eps
        ctx.precision = precision
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, z, y, gamma, running_mean, running_var = ctx.saved_tensors
        dz, dgamma, dbeta = T.bn_relu_eval_backward(dy.contiguous(), y, z, gamma.detach().contiguous(), running_mean,
                                                    running_var, ctx.eps)
        dw, db = T.conv_wgrad(x, dz, w.shape, precision=ctx.precision)
        dx = (T.conv_dgrad(dz, w.detach().contiguous(), precision=ctx.precision) if ctx.needs_input_grad[0]
              else None)
        return dx, dw, db, dgamma, dbeta, None, None, None, None


class _UntiedBias1x1(torch.nn.Module):
    """The reference's Conv2dUntiedBias(9, 9, 128, 1, 1) (nnet.py:138-180): weight [1,128,1,1], bias [1,9,9]."""

    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(1, 128, 1, 1))
        self.bias = torch.nn.Parameter(torch.empty(1, 9, 9))
        stdv = 1.0 / math.sqrt(128)
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            self.bias.uniform_(-stdv, stdv)

    def forward(self, h):
        # a sum over channels, not F.conv2d: no MIOpen algorithm choice on the path
        return (h * self.weight.reshape(1, 128, 1, 1)).sum(1, keepdim=True) + self.bias.unsqueeze(0)


def _trunk_modules():
    """nn.Sequential with the reference's indices: 0,3,..,18 Conv2d, 1,4,..,19 BatchNorm2d, 2,5,..,20 ReLU, 21 head.
    The Conv2d modules only hold parameters (and give torch's default initialisation); forward() never calls them."""
    mods = []
    for l in range(N_TRUNK):
        k = 5 if l == 0 else 3
        mods += [torch.nn.Conv2d(27 if l == 0 else 128, 128, k, padding=k // 2), torch.nn.BatchNorm2d(128),
                 torch.nn.ReLU()]
    return torch.nn.Sequential(*mods, _UntiedBias1x1())


def _as_state_dict(sd):
    """torch state_dict, BKW arrays (bkw.load_bkw) or a {"model_state_dict": ...} checkpoint -> torch state_dict."""
    if "model_state_dict" in sd:
        sd = sd["model_state_dict"]
    out = {}
    for k, v in sd.items():
        out[k] = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v))
    for c, b in zip(_CONV, _BN):
        out.setdefault(f"conv.{b}.num_batches_tracked", torch.tensor(0, dtype=torch.int64))
    for n in ("bn", "lin_bn"):
        if f"{n}.running_var" in out:
            out.setdefault(f"{n}.num_batches_tracked", torch.tensor(0, dtype=torch.int64))
    return out


def load_weights(path):
    """A .bkw file or a .pt file (a checkpoint or a bare state_dict) -> torch state_dict on the CPU."""
    if path.endswith(".bkw"):
        from .bkw import load_bkw
        return _as_state_dict(load_bkw(path))
    return _as_state_dict(torch.load(path, map_location="cpu"))


def _check_precision(precision):
    if precision not in T.PRECISIONS:
        raise ValueError(f"precision must be one of {T.PRECISIONS}, got {precision!r}")
    return precision


class _Trainable(torch.nn.Module):
    """precision: "fp32", or "bf16" for the trunk convolutions on bf16 operands with fp32 accumulation (forward and
    both gradients; weights, activations, BatchNorm, heads and the optimizer stay fp32).  A plain attribute of the
    run: it may be changed on a live net and is not part of state_dict()."""

    def __init__(self, device="cuda", precision="fp32"):
        super().__init__()
        self.precision = _check_precision(precision)
        self.conv = _trunk_modules()
        self.to(device)

    @classmethod
    def from_state_dict(cls, sd, device="cuda", precision="fp32"):
        """sd: a torch state_dict with the reference's names, BKW arrays, or a checkpoint dict."""
        net = cls(device=device, precision=precision)
        net.load_state_dict(_as_state_dict(sd))
        return net

    def trunk(self, x):
        """x [B,27,9,9] (float32 or uint8 planes) -> [B,1,9,9], the output of conv.21."""
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if not x.is_cuda:
            raise ValueError("the trainable nets run on the GPU: move the planes there first")
        h = x.float().contiguous()
        prec = _check_precision(self.precision)
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.conv.parameters())
        for l in range(N_TRUNK):
            conv, bn = self.conv[3 * l], self.conv[3 * l + 1]
            if self.training:
                h = _TrunkBlock.apply(h, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                      bn.num_batches_tracked, bn.momentum, bn.eps, prec)
            elif grad:  # eval mode with gradients (REINFORCE): frozen running statistics, differentiated
                h = _TrunkBlockEval.apply(h, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
                                          bn.running_var, bn.eps, prec)
            else:  # eval mode under no_grad: running statistics, no autograd
                z = T.conv_forward(h, conv.weight.detach().contiguous(), conv.bias.detach().contiguous(),
                                   precision=prec)
                h = T.bn_relu_eval(z, bn.weight.detach().contiguous(), bn.bias.detach().contiguous(), bn.running_mean,
                                   bn.running_var, bn.eps)
        return self.conv[21](h)


class TrainablePolicyNet(_Trainable):
    """(B,27,9,9) -> (B,81) logits; PolicyNet (nnet.py:19-57) with gradients."""

    def forward(self, x):
        return self.trunk(x).reshape(-1, 81)


class TrainableValueNet(_Trainable):
    """(B,27,9,9) -> (B,1) in (-1,1); ValueNet (nnet.py:59-113) with gradients."""

    def __init__(self, device="cuda", precision="fp32"):
        torch.nn.Module.__init__(self)
        self.precision = _check_precision(precision)
        self.conv = _trunk_modules()
        self.lin1 = torch.nn.Linear(81, 64)
        self.lin2 = torch.nn.Linear(64, 1)
        self.bn = torch.nn.BatchNorm2d(1)
        self.lin_bn = torch.nn.BatchNorm1d(64)
        self.to(device)

    def load_policy_dict(self, policy_dict):
        """Overlay a PolicyNet state_dict onto the trunk (nnet.py:103-107)."""
        new = self.state_dict()
        new.update({k: v for k, v in _as_state_dict(policy_dict).items() if k in new})
        self.load_state_dict(new)
        return self

    def forward(self, x):
        z = self.trunk(x)
        with torch.backends.cudnn.flags(enabled=False):  # torch's own BatchNorm kernels, not MIOpen's
            h = F.relu(self.bn(z)).reshape(-1, 81)
            h = F.relu(self.lin_bn(self.lin1(h)))
        return torch.tanh(self.lin2(h))


# ---- records -> positions -----------------------------------------------------------------------------------------
def _dihedral():
    """perm[g][d] = the source point that lands on point d under symmetry g (g = 4 * flip + quarter turns)."""
    perms = np.empty((8, 81), np.int64)
    for g in range(8):
        for q in range(81):
            r, c = divmod(q, 9)
            if g >= 4:
                c = 8 - c
            for _ in range(g % 4):
                r, c = c, 8 - r
            perms[g][9 * r + c] = q
    return perms


DIHEDRAL = _dihedral()
DIHEDRAL_INVERSE = np.argsort(DIHEDRAL, axis=1)  # DIHEDRAL[g][DIHEDRAL_INVERSE[g]] is the identity


def apply_symmetry(planes, g):
    """planes [..., 9, 9] or [..., 81] (numpy) -> the same under symmetry g."""
    shp = planes.shape
    flat = planes.reshape(shp[:-2] + (81,)) if shp[-2:] == (9, 9) else planes
    return flat[..., DIHEDRAL[g]].reshape(shp)


def find_records(paths):
    """Every games.json under the given files / directories (selfplay --out's rank*/ layout), sorted."""
    out = []
    for p in paths:
        if os.path.isfile(p):
            out.append(p)
            continue
        for root, dirs, files in os.walk(p):
            dirs.sort()
            if "games.json" in files:
                out.append(os.path.join(root, "games.json"))
    if not out:
        raise FileNotFoundError(f"no games.json under {list(paths)}")
    return out


class RecordDataset:
    """Positions of self-play records, one per ply, replayed with go.Game.play_move.

    planes     uint8 [N,27,9,9]  features_u8() of the position before the move: the incremental planes the search saw
    policy     float32 [N,81]    the root's visit counts at that ply normalised, or the played move one-hot when no
                                 visits were recorded; zero on pass plies
    has_policy bool [N]          False on pass plies (no policy target)
    value      float32 [N]       +1 if the side to move won the game (score > 0: black won), else -1 -- the sign
                                 convention of the value net (+ = good for the side to move, nnet.py:59-65)
    """

    def __init__(self, paths, augment=False, seed=0):
        if isinstance(paths, str):
            paths = [paths]
        self.files = find_records(paths)
        self.augment, self.seed = bool(augment), int(seed)
        planes, pol, has, val, self.game_of = [], [], [], [], []
        for fi, path in enumerate(self.files):
            with open(path) as f:
                rec = json.load(f)
            for gid in sorted(rec, key=int):
                g_rec = rec[gid]
                moves, visits = g_rec["moves"], g_rec.get("visits")
                black_won = g_rec["score"] > 0
                game = go.Game()
                for ply, mv in enumerate(moves):
                    planes.append(game.features_u8())
                    black_to_move = game.turn % 2 == 0
                    val.append(1.0 if black_to_move == black_won else -1.0)
                    p = np.zeros(81, np.float32)
                    if mv != go.PASS:
                        v = visits[ply] if visits else None
                        if v:
                            n = {int(k): float(c) for k, c in v.items() if 0 <= int(k) < 81 and c > 0}
                            tot = sum(n.values())
                            for k, c in n.items():
                                p[k] = c / tot
                        if not p.any():
                            p[mv] = 1.0
                    pol.append(p)
                    has.append(mv != go.PASS)
                    self.game_of.append((fi, int(gid), ply))
                    game.play_move(mv)
        self.planes = np.stack(planes) if planes else np.zeros((0, 27, 9, 9), np.uint8)
        self.policy = np.stack(pol) if pol else np.zeros((0, 81), np.float32)
        self.has_policy = np.array(has, bool)
        self.value = np.array(val, np.float32)

    def __len__(self):
        return len(self.value)

    def __getitem__(self, i):
        return self.planes[i], self.policy[i], self.has_policy[i], self.value[i]

    def batches(self, batch_size, epoch=0, device="cuda", shuffle=True):
        """Device tensors (planes u8, policy, has_policy, value) of `batch_size` positions, seeded by (seed, epoch);
        with augment, each position goes through its own seeded dihedral symmetry.  A last batch smaller than
        2 is dropped (train-mode BatchNorm needs a batch)."""
        rng = np.random.default_rng([self.seed, int(epoch)])
        order = rng.permutation(len(self)) if shuffle else np.arange(len(self))
        perms = torch.from_numpy(DIHEDRAL).to(device)
        for s in range(0, len(order), batch_size):
            idx = order[s:s + batch_size]
            if len(idx) < 2:
                break
            x = torch.from_numpy(self.planes[idx]).to(device)
            p = torch.from_numpy(self.policy[idx]).to(device)
            if self.augment:
                pg = perms[torch.from_numpy(rng.integers(0, 8, len(idx))).to(device)]  # [b, 81]
                x = torch.gather(x.reshape(len(idx), 27, 81), 2, pg.unsqueeze(1).expand(-1, 27, -1)).reshape(x.shape)
                p = torch.gather(p, 1, pg)
            yield (x, p, torch.from_numpy(self.has_policy[idx]).to(device), torch.from_numpy(self.value[idx]).to(device))


class ValueRecordDataset(RecordDataset):
    """The rows of genvals CSV files (board,ko,last,turn,val), value targets only.

    planes     uint8 [N,27,9,9]  bk_pos_from_board(board, ko, last, turn) + bk_pos_features_u8(fresh=1): the reference's
                                 Game(board=...), whose liberties are recomputed from the board
    policy     float32 [N,81]    zero; has_policy is False everywhere
    value      float32 [N]       val (+1 / -1 from the side to move)
    """

    def __init__(self, paths, augment=False, seed=0):
        from .genvals import read_rows

        if isinstance(paths, str):
            paths = [paths]
        self.files = list(paths)
        self.augment, self.seed = bool(augment), int(seed)
        planes, val, self.game_of = [], [], []
        for fi, path in enumerate(self.files):
            for i, (board, ko, last, turn, v) in enumerate(read_rows(path)):
                if v not in (1, -1):
                    raise ValueError(f"{path}: row {i}: val must be +1 or -1, got {v}")
                g = go.Game(board=board, ko=None if ko < 0 else ko, last_move=last, turn=turn)
                planes.append(g.features_u8(fresh=True))
                val.append(float(v))
                self.game_of.append((fi, i, -1))
        self.planes = np.stack(planes) if planes else np.zeros((0, 27, 9, 9), np.uint8)
        self.policy = np.zeros((len(val), 81), np.float32)
        self.has_policy = np.zeros(len(val), bool)
        self.value = np.array(val, np.float32)


def merge_datasets(first, *rest):
    """One dataset holding the positions of all, in order; batches() as first's (augment, seed)."""
    out = object.__new__(RecordDataset)
    parts = (first,) + rest
    out.files = [f for d in parts for f in d.files]
    out.augment, out.seed = first.augment, first.seed
    out.game_of = [g for d in parts for g in d.game_of]
    for name in ("planes", "policy", "has_policy", "value"):
        setattr(out, name, np.concatenate([getattr(d, name) for d in parts]))
    return out


# ---- losses and the training loop ---------------------------------------------------------------------------------
def policy_loss(logits, target, mask=None):
    """-sum pi * log_softmax(logits), averaged over the positions with a target (the reference's CrossEntropyLoss
    for one-hot pi)."""
    per = -(target * F.log_softmax(logits, dim=1)).sum(1)
    if mask is None:
        return per.mean()
    m = mask.float()
    return (per * m).sum() / m.sum().clamp_min(1.0)


def value_loss(out, target):
    """MSE, as bin/train.py."""
    return F.mse_loss(out.reshape(-1), target.reshape(-1))


def save_checkpoint(path, net, opt, epoch):
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in net.state_dict().items()},
                "optimizer_state_dict": opt.state_dict(), "epoch": int(epoch)}, path)


def _is_value_dict(sd):
    return "lin1.weight" in sd


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the policy / value nets from self-play records on the MI355X")
    ap.add_argument("--records", nargs="+", default=None, help="directories (searched for games.json) or files")
    ap.add_argument("--values", nargs="+", default=None,
                    help="genvals CSV files: value targets, trained together with those of --records")
    ap.add_argument("--net", choices=["policy", "value", "both"], default="both")
    ap.add_argument("-c", dest="checkpoint", nargs="+", default=[],
                    help="resume from policy_N.pt / value_N.pt (model + optimizer + epoch; a bare state_dict or a .bkw "
                         "gives the weights only); each file goes to the net its keys belong to")
    ap.add_argument("--init-trunk-from", default=None,
                    help="policy weights (.pt / .bkw) for the trunk of the nets trained (ValueNet.load_policy_dict)")
    ap.add_argument("-e", "--epochs", type=int, default=1)
    ap.add_argument("-b", "--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=0.0, help="> 0 switches Adam to AdamW")
    ap.add_argument("--augment", action="store_true", help="a seeded random dihedral symmetry per position")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=".")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--precision", choices=list(T.PRECISIONS), default="fp32",
                    help="bf16: the trunk convolutions on bf16 operands with fp32 accumulation; checkpoints stay fp32")
    args = ap.parse_args(argv)
    if args.batch < 2:
        ap.error("-b must be at least 2: BatchNorm in train mode needs a batch")
    if args.epochs < 1:
        ap.error("-e must be at least 1")
    if not args.records and not args.values:
        ap.error("give --records and/or --values")
    if args.values and not args.records and args.net != "value":
        ap.error("--values holds value targets only: without --records use --net value")

    torch.manual_seed(args.seed)
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    if args.values:
        parts = [RecordDataset(args.records, augment=args.augment, seed=args.seed)] if args.records else []
        parts.append(ValueRecordDataset(args.values, augment=args.augment, seed=args.seed))
        data = merge_datasets(*parts)
    else:
        data = RecordDataset(args.records, augment=args.augment, seed=args.seed)
    if len(data) < 2:
        raise SystemExit("fewer than 2 positions in the records")
    names = ["policy", "value"] if args.net == "both" else [args.net]
    nets = {n: (TrainablePolicyNet if n == "policy" else TrainableValueNet)(device=dev, precision=args.precision)
            for n in names}
    if args.init_trunk_from:
        trunk = load_weights(args.init_trunk_from)
        for n, net in nets.items():
            if n == "value":
                net.load_policy_dict(trunk)
            else:
                net.load_state_dict({k: v for k, v in trunk.items() if k in net.state_dict()})
    opt_cls = torch.optim.AdamW if args.weight_decay > 0 else torch.optim.Adam
    opts = {n: opt_cls(net.parameters(), lr=args.lr, weight_decay=args.weight_decay) for n, net in nets.items()}
    start = {n: 0 for n in names}
    for path in args.checkpoint:
        ck = torch.load(path, map_location="cpu") if not path.endswith(".bkw") else {}
        sd = load_weights(path)
        n = "value" if _is_value_dict(sd) else "policy"
        if n not in nets:
            raise SystemExit(f"{path} is a {n} checkpoint, but --net {args.net}")
        nets[n].load_state_dict(sd)
        if "optimizer_state_dict" in ck:
            opts[n].load_state_dict(ck["optimizer_state_dict"])
        start[n] = int(ck.get("epoch", 0))
    os.makedirs(args.out, exist_ok=True)

    for e in range(args.epochs):
        for net in nets.values():
            net.train()
        sums = {n: 0.0 for n in names}
        steps, positions = 0, 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for x, p, has, v in data.batches(args.batch, epoch=start[names[0]] + e, device=dev):
            losses = {}
            if "policy" in nets and not (args.values and not bool(has.any())):  # a batch of --values rows only
                losses["policy"] = policy_loss(nets["policy"](x), p, has)
            if "value" in nets:
                losses["value"] = value_loss(nets["value"](x), v)
            for n, loss in losses.items():
                opts[n].zero_grad(set_to_none=True)
                loss.backward()
                opts[n].step()
                sums[n] += loss.detach()
            steps += 1
            positions += len(v)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        line = {"epoch": None, "steps": steps, "positions": positions, "positions_per_s": positions / dt,
                "seconds": dt, "precision": args.precision}
        for n in names:
            ep = start[n] + e + 1
            path = os.path.join(args.out, f"{n}_{ep}.pt")
            save_checkpoint(path, nets[n], opts[n], ep)
            line["epoch"] = ep
            line[f"{n}_loss"] = float(sums[n]) / max(steps, 1)
            line[f"{n}_checkpoint"] = path
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

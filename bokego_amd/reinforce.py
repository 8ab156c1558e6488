"""REINFORCE on policy-vs-policy games against a pool of earlier policies (the reference's bin/selfplay.py:59-208).

    python -m bokego_amd.reinforce -w WEIGHTS_DIR [-e E] [-n N] [-b B] [--workers W] [-f STATS] [--lr 1e-5] [--seed S]
                                   [--opponent ID|random] [--device D] [--precision fp32|bf16] [--finish]

The pool is the policy_<id>.pt / .bkw files of -w.  With n = (number of ids) - 1, policy_n is trained; each epoch it
plays an opponent from the pool (policy_0 when it exists), writes policy_{n+1}.pt and three lines of statistics, and n
grows by one.  An iteration plays W batches of b games in lock-step -- the learner is black in even batches and white
in odd ones -- with the learner's weights as they stood at the start of the iteration, then takes one AdamW step per
batch, in batch order, on

    loss_batch = (1/b) * sum_games r_g * sum_{learner's plies} -log pi(a|s),     r_g = +1 if the learner won, else -1.

Playouts (play_games) are device-resident from the first ply to the scores.  The games are laid out once so that the
learner-is-black and the learner-is-white games are two contiguous slices of the uint8 [G, 192] bk_pos record tensor
and of the planes.  Per ply: one fp32 LeafEngine.eval_device per side on its slice, bkt_sample_moves on the logits, a
copy of the learner's slice (planes, moves, logp) into preallocated row buffers, and one bkt_play_moves that plays the
moves and writes the next ply's planes: no host work, no download and no synchronisation per ply.  bkt_area_score scores
the final records, and one download brings back the move history and the scores.  The learner's rows stay on the
device and are the update's batch.  play_games(rules="host") is the same loop with the rules on the host (per ply
lockstep.features_batch on the live games' records, one upload, 4 bytes per game back, lockstep.play_host, and
lockstep.area_score_host at the end): the reference the tests and the benchmark compare against, identical in every
output.  The host mirrors of the sampler and the host rules live in lockstep.py, shared with genvals and rollout.

The update differentiates the network that sampled the moves: the eval-mode TrainablePolicyNet, BatchNorm with its
running statistics frozen (train._TrunkBlockEval), which is the function the engine computes with the statistics
folded in.  Randomness comes only from Philox4x32-10 keyed by --seed with counter (game, ply, iteration, epoch), so
the same seed and pool give the same checkpoints bit for bit.  DESIGN 12 lists where this departs from the reference.

--finish (play_games(finish=True)): after the last sampled ply the games are played out to two passes in a row
(rollout.finish_games, pair form: the learner and the opponent keep their colours, the counters run on with the ply),
and black_wins / reward come from the area score of the finished boards, on which dead stones have been captured.
The finishing plies contribute no rows to the update.  A game whose turn lags (a side had no legal point at some ply)
is left out and scored as it stands.

--precision bf16 puts the update's trunk convolutions on bf16 operands (train._Trainable.precision).  The
playouts keep sampling from the fp32 engine, so the update then differentiates a function whose logits differ slightly
from the ones the moves were sampled from.
"""
import argparse
import json
import os
import re
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import _trainlib as T
from . import go
from . import lockstep as L
from .lockstep import (KOMI, LEGAL_PLANE, PLANE_BYTES, POS_BYTES, _play_fn, cdf_margin,  # noqa: F401  (the shared
                       degenerate_rows, features_batch, initial_positions, philox4x32_10,  # pieces, under the names the
                       sample_host, seed_key, uniform)                                   # tests and tools know)
from .selfplay import POLICY_MAX_TURNS

UPDATE_CHUNK = 32768       # rows per forward/backward of the update (libbktrain's trunk takes up to 65536)


def counters(game_ids, ply, iteration, epoch):
    """The counter words (game id, ply, iteration, epoch) of each game, as int32 [n, 4] (the bits the kernel reads)."""
    g = np.asarray(game_ids, np.int64)
    c = np.empty((len(g), 4), np.uint32)
    c[:, 0] = g
    c[:, 1] = int(ply)
    c[:, 2] = int(iteration)
    c[:, 3] = int(epoch)
    return c.view(np.int32)


# ---- the loss ----------------------------------------------------------------------------------------------------------
def reinforce_loss(logp, row_game, rewards, batch_size):
    """(1/b) * sum_g r_g * sum_{rows of g} -logp: logp [R] log pi(a|s) of the learner's rows, row_game [R] the game
    (0..b-1) of each row, rewards [b] +1 / -1 from the learner's side."""
    return -(rewards[row_game] * logp).sum() / batch_size


# ---- the pool ---------------------------------------------------------------------------------------------------------
_POLICY_FILE = re.compile(r"policy_(\d+)\.(pt|bkw)$")


def policy_pool(wdir):
    """{id: path} of the policy_<id>.pt / policy_<id>.bkw files in wdir (.pt wins when both exist)."""
    pool = {}
    for name in sorted(os.listdir(wdir)):
        m = _POLICY_FILE.fullmatch(name)
        if m and (int(m[1]) not in pool or m[2] == "pt"):
            pool[int(m[1])] = os.path.join(wdir, name)
    return pool


def learner_id(pool, wdir="."):
    """n = (number of policies) - 1, the reference's pool numbering (selfplay.py:144-148); policy_n must exist."""
    if not pool:
        raise FileNotFoundError(f"no policy_<id>.pt or .bkw in {wdir}")
    n = len(pool) - 1
    if n not in pool:
        raise FileNotFoundError(f"{len(pool)} policies in {wdir} but no policy_{n}: the pool must be numbered 0..{n}")
    return n


def choose_opponent(pool, n, seed, epoch, opponent=None):
    """policy_0 when it exists, else a seeded uniform choice among the ids 0..n present (selfplay.py:160-166);
    opponent: an id of the pool, or "random" for the seeded choice even when policy_0 exists."""
    ids = sorted(i for i in pool if i <= n)
    if opponent is not None and opponent != "random":
        if int(opponent) not in pool:
            raise FileNotFoundError(f"--opponent {opponent}: no policy_{opponent} in the pool")
        return int(opponent)
    if opponent is None and 0 in pool:
        return 0
    rng = np.random.default_rng([L.seed_u64(seed), int(epoch)])
    return ids[int(rng.integers(len(ids)))]


def stats_lines(n, opp, batch_size, iterations, wins):
    """The three lines the reference appends per epoch (selfplay.py:201-204)."""
    return [f"Policy {n} vs. Policy {opp}", f"Batch Size: {batch_size}, Iterations: {iterations}",
            ",".join(str(int(w)) for w in wins)]


# ---- lock-step playouts ------------------------------------------------------------------------------------------------
class Playouts:
    """What play_games returns.

    moves         int16 [G, 71]  the moves of each game (PASS = -1 pads after its end), game g in batch g // b
    length        int [G]        plies played
    black_wins    bool [G]       area score with komi 5.5 > 0
    learner_black bool [G]       the learner plays black (even batches)
    reward        float32 [G]    +1 / -1 from the learner's side
    planes        uint8 [R,27,9,9] on the device: the positions where the learner moved, in ply order, games ascending
    played        int64 [R] on the device: the learner's move in each
    logp          float32 [R] on the device: bkt_sample_moves' log-probability of it
    row_game      int64 [R] (host): the game of each row
    """

    def batch_rows(self, w, b):
        """Device index of the rows of batch w (games w*b .. w*b + b - 1) and their games within the batch."""
        sel = np.nonzero(self.row_game // b == w)[0]
        dev = self.planes.device
        return torch.from_numpy(sel).to(dev), torch.from_numpy(self.row_game[sel] - w * b).to(dev)


def _start_positions(start, G):
    """The records play_games starts from, uint8 [G, 192] (a copy): empty boards, or `start` checked."""
    if start is None:
        return L.initial_positions(G)
    if isinstance(start, torch.Tensor):
        start = start.cpu().numpy()
    start = np.array(start, order="C")
    if start.dtype != np.uint8 or start.shape != (G, POS_BYTES):
        raise ValueError(f"start must be uint8 [{G}, {POS_BYTES}], got {start.dtype} {start.shape}")
    turn = L.record_turns(start)
    if (turn != 0).any():
        raise ValueError(f"start: record {int(np.nonzero(turn)[0][0])} has turn {int(turn[turn != 0][0])}; every record "
                         "must have turn 0 (black to move), so that the ply equals the turn")
    return start


def _check_logp(games):
    """games: the games with a kept row whose logp is NaN (bkt_sample_moves' mark of a degenerate row)."""
    if len(games):
        raise FloatingPointError(f"game {int(np.min(games))}: the policy's logits are not finite (a NaN, a +inf or a "
                                 f"row of -inf: the sampler drew nothing there), in {len(np.unique(games))} game(s)")


def _finish(recs, perm, nb, plies, learner, opponent, key, iteration, epoch, dev, rules):
    """play_games(finish=True): play out the records recs (slot order: perm[slot] = game, the learner black in slots
    [0, nb)) whose turn is `plies` -> (the slots played out, rollout.Finished)."""
    from . import rollout
    turn = L.record_turns(recs)
    if isinstance(turn, torch.Tensor):
        turn = turn.cpu().numpy()
    sel = np.nonzero(turn == plies)[0]
    if len(sel) == 0:
        return sel, None
    sub = recs.index_select(0, torch.from_numpy(sel).to(recs.device)) if isinstance(recs, torch.Tensor) else recs[sel]
    fin = rollout.finish_games(sub, (learner, opponent), key, counters=counters(perm[sel], plies, iteration, epoch),
                               sides=(int((sel < nb).sum()),), rules=rules, device=dev, komi=KOMI)
    return sel, fin


def _play_games_device(learner, opponent, n_batches, batch_size, key, iteration, epoch, dev, timing, max_turns, pos0,
                       finish=False):
    """play_games(rules="device"): see the module docstring."""
    G, T_ = n_batches * batch_size, max_turns + 1
    learner_black = (np.arange(G) // batch_size) % 2 == 0
    perm = np.concatenate([np.nonzero(learner_black)[0], np.nonzero(~learner_black)[0]])   # slot -> game
    nb = int(learner_black.sum())
    side = (slice(0, nb), slice(nb, G))                   # slots of the learner-is-black / learner-is-white games
    lap = L.phase_clock(dev, timing)
    t = time.perf_counter()
    pos = torch.from_numpy(pos0[perm]).to(dev)
    ctr = torch.from_numpy(counters(perm, 0, iteration, epoch)).to(dev)
    planes = torch.empty((G, 27, 9, 9), dtype=torch.uint8, device=dev)
    hist = torch.full((G, T_), go.PASS, dtype=torch.int16, device=dev)
    status = T.play_moves(pos, torch.full((G,), -1, dtype=torch.int32, device=dev), planes)    # ply 0's planes
    # the learner's rows in ply order: ply p holds the games of side p % 2, ascending
    n_side = (nb, G - nb)
    row0 = np.concatenate([[0], np.cumsum([n_side[p % 2] for p in range(T_)])])
    rows_planes = torch.empty((int(row0[-1]), 27, 9, 9), dtype=torch.uint8, device=dev)
    rows_moves = torch.empty((int(row0[-1]),), dtype=torch.int32, device=dev)
    rows_logp = torch.empty((int(row0[-1]),), dtype=torch.float32, device=dev)
    t = lap("rules", t)
    for ply in range(T_):
        mine = side[ply % 2]
        if ply:
            ctr[:, 1].fill_(ply)
        engines = (learner, opponent) if ply % 2 == 0 else (opponent, learner)      # black is to move on even plies
        logits = L.engine_logits([(eng, planes[sl]) for eng, sl in zip(engines, side)])
        t = lap("engine", t)
        moves, logp = T.sample_moves(logits, planes, key, ctr)
        hist[:, ply] = moves
        t = lap("sampler", t)
        a, b = int(row0[ply]), int(row0[ply + 1])
        if b > a:                                         # before bkt_play_moves overwrites the planes
            rows_planes[a:b] = planes[mine]
            rows_moves[a:b] = moves[mine]
            rows_logp[a:b] = logp[mine]
        status |= T.play_moves(pos, moves, planes)
        t = lap("rules", t)
    score = T.area_score(pos, KOMI)
    t = lap("score", t)
    finished = None
    if finish:
        sel, fin = _finish(pos, perm, nb, T_, learner, opponent, key, iteration, epoch, dev, "device")
        if fin is not None:
            score[torch.from_numpy(sel).to(dev)] = torch.from_numpy(fin.score).to(dev)
        finished = (perm[sel], fin)
        t = lap("finish", t)
    # per slot, the kept rows (a move was played) whose logp is NaN: one more column of the one download
    row_slot = torch.from_numpy(np.concatenate([np.arange(G)[side[p % 2]] for p in range(T_)])).to(dev)
    nan_rows = torch.zeros(G, dtype=torch.int32, device=dev).index_add_(
        0, row_slot, (torch.isnan(rows_logp) & (rows_moves >= 0)).to(torch.int32))
    back = torch.cat([hist, score.view(torch.int16).view(G, 2), status.view(torch.int16).view(G, 2),
                      nan_rows.to(torch.int16).view(G, 1)], 1).cpu().numpy()
    t = lap("download", t)
    _check_logp(perm[np.nonzero(back[:, T_ + 4])[0]])
    st = np.ascontiguousarray(back[:, T_ + 2:T_ + 4]).view(np.int32)[:, 0]
    L.check_status(st, lambda s, v: f"game {perm[s]}: a sampled move is illegal (status {v}); the legal plane and the "
                   "rules disagree")
    out = Playouts()
    if finish:
        out.finished_games, out.finished = finished
    out.moves = np.empty((G, T_), np.int16)
    out.moves[perm] = back[:, :T_]
    scores = np.empty(G, np.float32)
    scores[perm] = np.ascontiguousarray(back[:, T_:T_ + 2]).view(np.float32)[:, 0]
    out.length = (out.moves >= 0).sum(1).astype(np.int64)        # a game without a move at a ply has none later
    out.learner_black = learner_black
    out.black_wins = scores > 0
    out.reward = np.where(out.black_wins == learner_black, 1.0, -1.0).astype(np.float32)
    row_game = np.concatenate([perm[side[p % 2]] for p in range(T_)]).astype(np.int64)
    keep = out.moves[row_game, np.repeat(np.arange(T_), [n_side[p % 2] for p in range(T_)])] >= 0
    if not keep.all():                                    # the plies of ended games
        k = torch.from_numpy(np.nonzero(keep)[0]).to(dev)
        rows_planes, rows_moves, rows_logp = (x.index_select(0, k) for x in (rows_planes, rows_moves, rows_logp))
        row_game = row_game[keep]
    out.planes, out.played, out.logp, out.row_game = rows_planes, rows_moves.long(), rows_logp, row_game
    lap("download", t)
    return out


def play_games(learner, opponent, n_batches, batch_size, seed, iteration=0, epoch=0, device=None, timing=None,
               max_turns=POLICY_MAX_TURNS, rules="device", start=None, finish=False):
    """n_batches * batch_size games in lock-step between two fp32 LeafEngines (policy weights); the learner is black in
    even batches.  rules="device": bkt_play_moves and bkt_area_score, nothing on the host per ply; "host": the host
    rules (lockstep: features_batch, the upload, play_host, area_score_host), the reference the tests and the benchmark
    compare against.  Both give the same Playouts, bit for bit.  start: uint8 [G, 192] bk_pos records to play from (game
    g from start[g]), every one with turn 0; default: empty boards.  timing: a dict that receives seconds per phase;
    the phases are then separated by synchronisations, so pass it only to measure.  Device rules: 'engine' (both
    evaluations), 'sampler' (bkt_sample_moves + the move history), 'rules' (the copy of the learner's rows +
    bkt_play_moves), 'score' (bkt_area_score), 'download'.  Host rules: 'host' (features, staging, playing the moves),
    'engine' (upload + both evaluations) and 'sampler' (bkt_sample_moves + the copy back).
    finish=True: the games are then played out to the end (rollout.finish_games with the same rules, phase 'finish') and
    black_wins / reward come from the finished boards; moves, length and the learner's rows are what they are without
    it.  The Playouts then also has finished_games (the games played out: all but those whose turn lags) and finished
    (their rollout.Finished, or None when there is none).
    FloatingPointError when the logp of a kept row is NaN, bkt_sample_moves' mark of a row whose logits are not finite
    (a diverged learner, a bad checkpoint): found where the results come to the host anyway, with no wait per ply."""
    L.check_rules(rules)
    G = n_batches * batch_size
    pos = _start_positions(start, G)
    dev = torch.device("cuda", learner.device_id) if device is None else torch.device(device)
    key = L.seed_u64(seed)
    if rules == "device":
        return _play_games_device(learner, opponent, n_batches, batch_size, key, iteration, epoch, dev, timing,
                                  max_turns, pos, finish)
    learner_black = (np.arange(G) // batch_size) % 2 == 0
    hist = np.full((G, max_turns + 1), go.PASS, np.int16)
    length = np.zeros(G, np.int64)
    staging = torch.empty(G * (16 + PLANE_BYTES), dtype=torch.uint8).pin_memory()
    stage = staging.numpy()
    rows_planes, rows_moves, rows_logp, rows_game = [], [], [], []
    live = np.arange(G)
    lap = L.phase_clock(dev, timing)
    t = time.perf_counter()
    for ply in range(max_turns + 1):
        if len(live) == 0:
            break
        mine = learner_black[live] == (ply % 2 == 0)
        order = np.concatenate([live[mine], live[~mine]])           # the learner's rows first
        nl, n = int(mine.sum()), len(order)
        recs = np.ascontiguousarray(pos[order])
        stage[:16 * n].view(np.int32)[:] = counters(order, ply, iteration, epoch).reshape(-1)
        L.features_batch(recs, stage[16 * n:].ctypes.data)
        t = lap("host", t)
        d = staging[:(16 + PLANE_BYTES) * n].to(dev, non_blocking=True)
        ctr = d[:16 * n].view(torch.int32).view(n, 4)
        planes = d[16 * n:].view(n, 27, 9, 9)
        logits = L.engine_logits([(learner, planes[:nl]), (opponent, planes[nl:])])
        t = lap("engine", t)
        d_moves, d_logp = T.sample_moves(logits, planes, key, ctr)
        moves = d_moves.cpu().numpy()
        t = lap("sampler", t)
        ok = moves >= 0
        L.play_host(recs, np.nonzero(ok)[0], moves[ok], lambda r, mv: f"game {order[r]} ply {ply}: sampled move {mv} is "
                    "illegal; the legal plane and the rules disagree")
        pos[order] = recs
        hist[order[ok], ply] = moves[ok]
        length[order[ok]] += 1
        if nl:
            keep = ok[:nl]
            if keep.all():
                rows_planes.append(planes[:nl])
                rows_moves.append(d_moves[:nl])
                rows_logp.append(d_logp[:nl])
            else:
                k = torch.from_numpy(np.nonzero(keep)[0]).to(dev)
                rows_planes.append(planes[:nl].index_select(0, k))
                rows_moves.append(d_moves[:nl].index_select(0, k))
                rows_logp.append(d_logp[:nl].index_select(0, k))
            rows_game.append(order[:nl][keep])
        live = np.sort(order[ok])                                   # turn > max_turns ends the game before its move
        t = lap("host", t)

    out = Playouts()
    out.moves, out.length, out.learner_black = hist, length, learner_black
    scores = L.area_score_host(pos, KOMI)
    if finish:
        perm = np.concatenate([np.nonzero(learner_black)[0], np.nonzero(~learner_black)[0]])
        sel, fin = _finish(np.ascontiguousarray(pos[perm]), perm, int(learner_black.sum()), max_turns + 1, learner,
                           opponent, key, iteration, epoch, dev, "host")
        if fin is not None:
            scores[perm[sel]] = fin.score
        out.finished_games, out.finished = perm[sel], fin
    out.black_wins = scores > 0
    out.reward = np.where(out.black_wins == learner_black, 1.0, -1.0).astype(np.float32)
    if rows_game:
        out.planes = torch.cat(rows_planes)
        out.played = torch.cat(rows_moves).long()
        out.logp = torch.cat(rows_logp)
        out.row_game = np.concatenate(rows_game).astype(np.int64)
        _check_logp(out.row_game[torch.isnan(out.logp).cpu().numpy()])      # once per call, after the last ply
    else:
        out.planes = torch.empty((0, 27, 9, 9), dtype=torch.uint8, device=dev)
        out.played = torch.empty((0,), dtype=torch.int64, device=dev)
        out.logp = torch.empty((0,), dtype=torch.float32, device=dev)
        out.row_game = np.zeros(0, np.int64)
    lap("host", t)
    return out


# ---- the learner -------------------------------------------------------------------------------------------------------
def played_logp(net, planes, played):
    """log pi(a|s) of the rows through the network (eval mode: the function the engine sampled from)."""
    logits = net(planes)
    return F.log_softmax(logits, dim=1).gather(1, played.reshape(-1, 1)).reshape(-1)


def update(net, opt, games, n_batches, batch_size, reward_override=None):
    """One AdamW step per batch, in batch order, on that batch's REINFORCE loss; -> the losses (floats).
    A batch without rows takes no step.  reward_override: +1 / -1 for every game (tests)."""
    net.eval()
    dev = games.planes.device
    reward = games.reward if reward_override is None else np.full_like(games.reward, reward_override)
    losses = []
    for w in range(n_batches):
        idx, gl = games.batch_rows(w, batch_size)
        if len(idx) == 0:
            losses.append(0.0)
            continue
        r = torch.from_numpy(np.ascontiguousarray(reward[w * batch_size:(w + 1) * batch_size])).to(dev)
        opt.zero_grad(set_to_none=True)
        loss = 0.0
        for s in range(0, len(idx), UPDATE_CHUNK):     # the loss is a sum over rows: gradients of chunks add up
            i = idx[s:s + UPDATE_CHUNK]
            part = reinforce_loss(played_logp(net, games.planes.index_select(0, i), games.played.index_select(0, i)),
                                  gl[s:s + UPDATE_CHUNK], r, batch_size)
            part.backward()
            loss += float(part.detach())
        opt.step()
        losses.append(loss)
    return losses


def wins_per_batch(games, n_batches, batch_size):
    return [int((games.reward[w * batch_size:(w + 1) * batch_size] > 0).sum()) for w in range(n_batches)]


def policy_engine(sd, device_id, max_batch):
    from .engine import LeafEngine
    return LeafEngine(sd, None, device_id=device_id, max_batch=max_batch, precision="f32")


def engine_weights(net):
    """The trainable net's state_dict in the form LeafEngine.set_weights takes."""
    return {k: v.detach() for k, v in net.state_dict().items()}


def _set_weights(learner_eng, net, iteration):
    """The updated weights into the learner's engine.  The engine refuses weights that are not finite (bk_engine_set_weights,
    BK_ERR_ARG naming the tensor) and goes on serving the old ones: here that is the end of the run, as in _check_logp."""
    try:
        learner_eng.set_weights(engine_weights(net))
    except ValueError as ex:
        if "not finite" not in str(ex):
            raise
        raise FloatingPointError(f"iteration {iteration}: the update left the policy's weights not finite "
                                 f"({str(ex).split('not finite: ')[-1]}); the engine keeps the weights it had") from ex


def run_epoch(net, opt, learner_eng, opp_eng, n_iters, n_batches, batch_size, seed, epoch, log=None, finish=False):
    """n_iters iterations: play, update, hand the new weights to the learner's engine.  -> wins per batch, in order."""
    wins = []
    for it in range(n_iters):
        t0 = time.perf_counter()
        games = play_games(learner_eng, opp_eng, n_batches, batch_size, seed, iteration=it, epoch=epoch, finish=finish)
        losses = update(net, opt, games, n_batches, batch_size)
        _set_weights(learner_eng, net, it)
        w = wins_per_batch(games, n_batches, batch_size)
        wins += w
        if log:
            log({"iteration": it, "wins": sum(w), "games": n_batches * batch_size, "rows": len(games.row_game),
                 "mean_loss": sum(losses) / len(losses), "seconds": time.perf_counter() - t0})
    return wins


def save_checkpoint(path, net, opt):
    """The reference's checkpoint: model_state_dict and optimizer_state_dict (selfplay.py:207-208)."""
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in net.state_dict().items()},
                "optimizer_state_dict": opt.state_dict()}, path)


def _parse(argv):
    ap = argparse.ArgumentParser(description="REINFORCE against a pool of earlier policies on the MI355X "
                                             "(the reference's bin/selfplay.py)")
    ap.add_argument("-w", dest="w", metavar="PATH", default=os.path.abspath(os.path.join("..", "data", "weights")),
                    help="the pool: policy_<id>.pt / .bkw files")
    ap.add_argument("-e", dest="e", metavar="E", type=int, default=1, help="number of epochs")
    ap.add_argument("-n", dest="n", metavar="N", type=int, default=64, help="iterations per epoch")
    ap.add_argument("-b", dest="b", metavar="B", type=int, default=16, help="games per batch")
    ap.add_argument("--workers", metavar="W", type=int, default=16,
                    help="batches per iteration (even: learner black, odd: white), one AdamW step each")
    ap.add_argument("-f", dest="f", metavar="PATH", default=os.path.join(os.getcwd(), "RL_stats.txt"),
                    help="file the statistics are appended to")
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--opponent", default=None, help="pool id of the opponent, or 'random' (default: policy_0 if any)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--precision", choices=list(T.PRECISIONS), default="fp32",
                    help="bf16: the update's trunk convolutions on bf16 operands with fp32 accumulation (the playouts "
                         "stay on the fp32 engine)")
    ap.add_argument("--finish", action="store_true",
                    help="play every game out to the end after the last sampled ply; rewards from the finished boards")
    args = ap.parse_args(argv)
    for flag, v in (("-e", args.e), ("-n", args.n), ("-b", args.b), ("--workers", args.workers)):
        if v < 1:
            ap.error(f"{flag} must be at least 1")
    if args.b * args.workers > 65536:
        ap.error("-b times --workers must be at most 65536 games")
    if args.opponent is not None and args.opponent != "random" and not re.fullmatch(r"\d+", args.opponent):
        ap.error("--opponent must be a pool id or 'random'")
    if not (0 <= args.seed < 2 ** 64):
        ap.error("--seed must be an unsigned 64-bit integer")
    if not os.path.isdir(args.w):
        ap.error(f"-w {args.w}: not a directory")
    return args


def main(argv=None):
    from .train import TrainablePolicyNet, load_weights

    args = _parse(argv)
    pool = policy_pool(args.w)
    n = learner_id(pool, args.w)
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    G = args.b * args.workers
    net = TrainablePolicyNet.from_state_dict(load_weights(pool[n]), device=dev, precision=args.precision).eval()
    opt = torch.optim.AdamW(net.parameters(), lr=args.lr)
    if pool[n].endswith(".pt"):
        ck = torch.load(pool[n], map_location="cpu")
        if isinstance(ck, dict) and "optimizer_state_dict" in ck:
            opt.load_state_dict(ck["optimizer_state_dict"])
    learner_eng = policy_engine(engine_weights(net), args.device, G)
    print(json.dumps({"pool": sorted(pool), "learner": n, "games_per_iteration": G}), flush=True)
    try:
        for _ in range(args.e):
            opp = choose_opponent(pool, n, args.seed, n, args.opponent)
            out = os.path.join(args.w, f"policy_{n + 1}.pt")
            if os.path.exists(out):
                raise SystemExit(f"{out} exists: the pool must be numbered 0..{n} with nothing above")
            opp_eng = policy_engine(load_weights(pool[opp]), args.device, G)
            t0 = time.perf_counter()
            try:
                wins = run_epoch(net, opt, learner_eng, opp_eng, args.n, args.workers, args.b, args.seed, n,
                                 log=lambda d: print(json.dumps(d), flush=True), finish=args.finish)
            finally:
                opp_eng.close()
            dt = time.perf_counter() - t0
            with open(args.f, "a+") as f:
                f.write("\n".join(stats_lines(n, opp, args.b, args.n, wins)) + "\n")
            save_checkpoint(out, net, opt)
            print(json.dumps({"epoch": n, "opponent": opp, "wins": sum(wins), "games": len(wins) * args.b,
                              "games_per_s": len(wins) * args.b / dt, "seconds": dt, "checkpoint": out}), flush=True)
            n += 1
            pool[n] = out
    finally:
        learner_eng.close()


if __name__ == "__main__":
    main()

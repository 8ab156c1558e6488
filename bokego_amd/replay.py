"""The lock-step replay of recorded games that the fits share: patterns.counts, tactics.counts, mmfit.pack,
mmfit.evaluate and balance.labelled_positions are bodies over the two walkers here, one on the host rules and one on the
device rules.  Beside them: the games a fit's command line replays (policy_games, record_games), the check of what a replay
takes, and the two decisions every body makes about the recorded move -- does it count, and where does the draw rank it.

The order is part of the result (a float sum, the rows of a pack): batches in ascending order of their first game, within a
batch the plies in ascending order, within a ply the live games in ascending order.
"""
import numpy as np
import torch

from . import _trainlib as T
from . import lockstep as L

MOVE_NONE = T.MOVE_NONE

__all__ = ["at_move", "check_games", "counted", "move_rank", "policy_games", "record_games", "replay_device", "replay_host"]


def check_games(start_recs, moves):
    """-> (start uint8 [G,192], moves int32 [G,L]), numpy; ValueError when the arguments are not records and their moves."""
    start = np.ascontiguousarray(start_recs.cpu().numpy() if isinstance(start_recs, torch.Tensor) else start_recs, np.uint8)
    moves = np.asarray(moves)
    if start.ndim != 2 or start.shape[1] != L.POS_BYTES or moves.ndim != 2 or len(moves) != len(start):
        raise ValueError("counts takes records uint8 [G,192] and their moves [G,L]")
    return start, moves.astype(np.int32)


# ---- the walkers ------------------------------------------------------------------------------------------------------------------
def replay_host(start, moves, batch=None, playable=True):
    """Walk the games of check_games on the host rules, `batch` games at a time (None: all at once).  Before every ply k
    at which a game of the batch is live (its move is above MOVE_NONE) it yields (k, first, live, recs, mv, ok): first the
    batch's first game, live the ascending rows of the batch that are live, recs uint8 [batch,192] the batch's records
    before the ply (the walker's own: read them, do not play on them), mv = moves[first + live, k], ok = playable_host(
    recs[live]) or None with playable=False.  Then it plays the moves, liberty cache included; a move the rules refuse
    raises RuntimeError naming the game."""
    for first in range(0, len(start), batch or max(len(start), 1)):
        recs, hist = start[first:first + (batch or len(start))].copy(), moves[first:first + (batch or len(start))]
        for k in range(hist.shape[1]):
            live = np.nonzero(hist[:, k] > MOVE_NONE)[0]
            if len(live) == 0:
                continue
            mv = hist[live, k]
            yield k, first, live, recs, mv, L.playable_host(recs[live]) if playable else None
            L.play_host(recs, live, mv, lambda g, m: f"game {first + g}: the recorded move {m} is illegal", liberties=True)


def replay_device(start, moves, dev, batch=T.MAX_BATCH, playable=True):
    """The same walk on the device rules: the records and the history of a batch are uploaded once, and before EVERY ply k
    it yields (k, first, pos, mv, live, ok): pos uint8 [batch,192] the records before the ply, mv int32 [batch] the moves,
    live bool [batch] = mv > MOVE_NONE, ok uint8 [batch,81] the playable sets bkt_playout_step left (None with
    playable=False) -- tensors on dev, the walker's own.  A ply costs the walker one bkt_playout_step (beside the copy of
    the history's column and its comparison) and no synchronisation; the status of the whole batch is read once at its end, RuntimeError naming the first refused game."""
    for first in range(0, len(start), batch):
        pos = torch.from_numpy(start[first:first + batch]).to(dev)
        hist = torch.from_numpy(moves[first:first + batch]).to(dev)
        ok = torch.empty((len(pos), 81), dtype=torch.uint8, device=dev) if playable else None
        if playable:                                                      # the playable sets of the start records
            status = T.playout_step(pos, torch.full((len(pos),), MOVE_NONE, dtype=torch.int32, device=dev), None, None, ok)
        else:
            status = torch.zeros(len(pos), dtype=torch.int32, device=dev)
        for k in range(hist.shape[1]):
            mv = hist[:, k].contiguous()
            yield k, first, pos, mv, mv > MOVE_NONE, ok
            status |= T.playout_step(pos, mv, None, None, ok)
        L.check_status(status, lambda g, st: f"game {first + g}: a recorded move is illegal (status {st})")


# ---- the recorded move ------------------------------------------------------------------------------------------------------------
def counted(mv, ok):
    """Does the move of each row count?  mv [n] and ok bool [n,81] (the points that may be counted: the playable ones),
    both numpy or both tensors -> (at int64 [n,1]: the move clipped onto the board, the column at_move takes; good bool
    [n]: the move is a board point and ok there).  A pass never counts, and neither does a move into the mover's own eye."""
    if isinstance(mv, torch.Tensor):
        at = mv.clamp(0, 80).to(torch.int64)[:, None]
    else:
        at = np.clip(mv, 0, 80).astype(np.int64)[:, None]
    return at, (mv >= 0) & at_move(ok, at)


def at_move(x, at):
    """x [n,81] at the column `at` [n,1] of every row -> [n] (numpy or tensors)."""
    return (x.gather(1, at) if isinstance(x, torch.Tensor) else np.take_along_axis(x, at, 1))[:, 0]


def move_rank(w, w_m, mv, ok):
    """How many candidates the draw ranks before the move of each row (numpy): w [n,81] the weights, w_m [n] the weight of
    the move, mv [n] the move, ok bool [n,81] the candidates.  Heavier ones, and equally heavy ones at a lower point."""
    return (ok & ((w > w_m[:, None]) | ((w == w_m[:, None]) & (np.arange(81)[None, :] < mv[:, None])))).sum(1)


# ---- the games of the command lines -------------------------------------------------------------------------------------------------
def policy_games(policy, games, seed, device):
    """`games` games of the policy net (weights .pt or .bkw) against itself from the empty board, sampled under `seed`
    and played to the end on `device` -> (start records uint8 [G,192], moves int16 [G,L])."""
    from . import rollout
    from .reinforce import policy_engine
    from .train import load_weights
    eng = policy_engine(load_weights(policy), device.index, min(games, 4096))
    try:
        start = L.initial_positions(games)
        return start, rollout.finish_games(start, eng, seed, device=device).moves
    finally:
        eng.close()


def record_games(paths):
    """The games of selfplay --out records (train.find_records) -> (start records uint8 [G,192], moves int16 [G,L])."""
    import json

    from .train import find_records
    games = []
    for path in find_records(paths):
        with open(path) as f:
            rec = json.load(f)
        games += [rec[g]["moves"] for g in sorted(rec, key=int)]
    moves = np.full((len(games), max(max(len(m) for m in games), 1)), MOVE_NONE, np.int16)
    for i, m in enumerate(games):
        moves[i, :len(m)] = m
    return L.initial_positions(len(games)), moves

"""Training data for the value net: positions labelled by the result of policy-vs-policy games (the reference's
bin/genvals.py).

    python -m bokego_amd.genvals -o values.csv [-w POOL | --sl PATH --rl PATH] [-n THOUSANDS | --games G]
                                 [--batch 4096] [--seed S] [--device D] [--finish]

A game (gen_game): r_g is drawn uniformly from [70, 90).  The SL policy samples plies 0 .. r_g - 1, ply r_g is a uniformly
random legal point, and the RL policy samples from then on while turn < 90.  The game is scored by area with komi 5.5.
The stored row is the position after the random move, labelled val = +1 if the side to move in it won, else -1 (the
value net's side-to-move convention).  A game in which SL, or the random move, finds no legal point is dropped.  An RL
game with no legal point is scored as it stands.  With -w, SL is the lowest id of the pool and RL the highest.

Playouts run in lock-step on the device, `--batch` games per pass.  The records are a uint8 [G, 192] tensor.  A pass
sorts its games by r_g once, so at ply p the RL rows (r_g < p), the rows at their random ply (r_g == p) and the SL rows
(r_g > p) are contiguous slices.  Each slice goes to its engine (or to the masked sampler) without a gather, and one
bkt_play_moves call per ply plays the moves and writes the next ply's planes.  bkt_area_score scores the final records.
Per pass the host downloads the kept records, the scores and the moves; it does no work and no synchronisation per ply.

Randomness comes only from Philox4x32-10 keyed by --seed (lockstep.philox4x32_10 is the numpy mirror).  Counters
depend on the game's global id g, never on its batch or row, so the output does not depend on --batch
(lockstep.game_counters, whose table names the streams):
    move at ply p (SL, random or RL):  (g mod 2^32, p, g >> 32, STREAM_MOVE)  -> bkt_sample_moves
    r_g:                               (g mod 2^32, 0, g >> 32, STREAM_R)     -> r_g = 70 + floor(20 * u), u = (x0 >> 8) * 2^-24
The random move is bkt_sample_moves on masked logits (0 on the legal points of plane 5, -inf elsewhere): the first
point whose prefix count of legal points exceeds u * (number of legal points), -1 when there is none.

--finish (generate(finish=True)): after turn 90 the RL policy plays the game out, both colours, to two passes in a row
(rollout.finish_games, the move counters running on with p = 90, 91, ...), and the label comes from
the area score of the finished board, on which dead stones have been captured.  The stored rows are the same; only
val can differ.

The output is a CSV with the header `board,ko,last,turn,val`, appended to (`a+`).  DESIGN 13 lists where this departs
from the reference.
"""
import argparse
import ctypes
import json
import os
import time

import numpy as np
import torch

from . import _trainlib as T
from . import go
from . import lockstep as L
from . import reinforce as R

MAX_TURNS = 90
R_LOW, R_HIGH = 70, 90           # r_g in [R_LOW, R_HIGH)
KOMI = L.KOMI
HEADER = "board,ko,last,turn,val"


# ---- counters (the numpy side of every draw) ------------------------------------------------------------------------------
def move_counters(game_ids, ply):
    """Counter words of the move at `ply` of each game, int32 [n, 4] (the bits bkt_sample_moves reads)."""
    return L.game_counters(game_ids, int(ply), L.STREAM_MOVE)


def random_ply(game_ids, seed):
    """r_g of each game: 70 + floor(20 u), u from the Philox draw of stream STREAM_R."""
    c = L.game_counters(game_ids, 0, L.STREAM_R).view(np.uint32)
    u = L.uniform(L.philox4x32_10(c, L.seed_key(seed))[:, 0])
    return (R_LOW + np.floor(u * (R_HIGH - R_LOW))).astype(np.int64)


def masked_logits(planes):
    """0 on the legal points (plane 5), -inf elsewhere: bkt_sample_moves then draws a uniformly random legal point."""
    legal = planes[:, L.LEGAL_PLANE].reshape(-1, 81) != 0
    return torch.zeros(legal.shape, dtype=torch.float32, device=planes.device).masked_fill_(~legal, float("-inf"))


# ---- the CSV --------------------------------------------------------------------------------------------------------------
def write_rows(path, rows):
    """Append rows (board, ko, last, turn, val) to path; the header goes in first when the file is new or empty.  A file
    whose first line is not the header is refused (ValueError) and left as it is."""
    with open(path, "a+") as f:
        f.seek(0)
        first = f.readline()
        if first and first.rstrip("\r\n") != HEADER:
            raise ValueError(f"{path}: header {first.rstrip()!r} is not {HEADER!r}")
        f.seek(0, os.SEEK_END)
        if not first:
            f.write(HEADER + "\n")
        for board, ko, last, turn, val in rows:
            f.write(f"{board},{int(ko)},{int(last)},{int(turn)},{int(val)}\n")


def read_rows(path):
    """-> list of (board str, ko int, last int, turn int, val int) from a file write_rows wrote."""
    rows = []
    with open(path) as f:
        first = f.readline().rstrip("\r\n")
        if first != HEADER:
            raise ValueError(f"{path}: header {first!r} is not {HEADER!r}")
        for n, line in enumerate(f, 2):
            line = line.strip()
            if not line:
                continue
            parts = line.split(",")
            if len(parts) != 5 or len(parts[0]) != 81:
                raise ValueError(f"{path}:{n}: expected board,ko,last,turn,val")
            rows.append((parts[0], int(parts[1]), int(parts[2]), int(parts[3]), int(parts[4])))
    return rows


# ---- the playouts -----------------------------------------------------------------------------------------------------------
class Generated:
    """What generate() returns, for games 0 .. G-1.

    rows   list of (board, ko, last, turn, val), one per kept game, games ascending
    game   int64 [K]         the game of each row
    r      int64 [G]         the random ply r_g
    moves  int16 [G, 90]     the move at each ply, -1 where none was played (after the end, or no legal point)
    score  float64 [G]       area score with komi 5.5 of the final position (> 0: black won)
    kept   bool [G]          SL and the random move found a legal point
    """


def _record_fields(recs):
    """board strings, ko, last move and turn of bk_pos records uint8 [n, 192]."""
    lib, buf = go.golib(), ctypes.create_string_buffer(82)
    boards = []
    for i in range(len(recs)):
        lib.bk_pos_board_string(L.pos_ptr(recs[i]), buf)
        boards.append(buf.value.decode("ascii"))
    return boards, *(f(recs).astype(np.int64) for f in (L.record_ko, L.record_last_move, L.record_turns))


def _pass(sl, rl, ids, seed, dev, rules, timing, finish=False):
    """One lock-step pass over the games `ids`, sorted by r_g -> (r, moves, kept records, area scores) in that order."""
    n = len(ids)
    r = random_ply(ids, seed)
    key = L.seed_u64(seed)
    empty_planes = torch.from_numpy(go.Game().features_u8()).to(dev)
    planes = empty_planes.unsqueeze(0).repeat(n, 1, 1, 1)
    ctr = torch.from_numpy(move_counters(ids, 0)).to(dev)
    moves = torch.empty((n,), dtype=torch.int32, device=dev)
    hist = torch.full((n, MAX_TURNS), -1, dtype=torch.int16, device=dev)
    init = L.initial_positions(n)
    if rules == "device":
        pos = torch.from_numpy(init).to(dev)
        kept = torch.empty_like(pos)
    else:
        pos, kept = init, np.empty_like(init)
        staging = torch.empty((n, 27, 9, 9), dtype=torch.uint8).pin_memory()
    lap = L.phase_clock(dev, timing)
    t = time.perf_counter()
    for ply in range(MAX_TURNS):
        rl_end = int(np.searchsorted(r, ply, "left"))     # rows [0, rl_end): RL; [rl_end, sl_start): random; rest: SL
        sl_start = int(np.searchsorted(r, ply, "right"))
        if ply:
            ctr[:, 1].fill_(ply)
        if rules == "host":
            L.features_batch(pos, staging.numpy().ctypes.data)
            planes.copy_(staging, non_blocking=True)
            t = lap("rules", t)
        logits = {}
        for name, eng, a, b in (("rl", rl, 0, rl_end), ("sl", sl, sl_start, n)):
            if b > a:
                logits[name] = L.engine_logits([(eng, planes[a:b])])
        t = lap("engine", t)
        for name, a, b in (("rl", 0, rl_end), ("rand", rl_end, sl_start), ("sl", sl_start, n)):
            if b > a:
                lg = masked_logits(planes[a:b]) if name == "rand" else logits[name]
                moves[a:b] = T.sample_moves(lg, planes[a:b], key, ctr[a:b])[0]
        hist[:, ply] = moves.to(torch.int16)
        t = lap("sampler", t)
        if rules == "device":
            T.play_moves(pos, moves, planes)
            if sl_start > rl_end:
                kept[rl_end:sl_start] = pos[rl_end:sl_start]
        else:
            mv = moves.cpu().numpy()
            L.play_host(pos, np.nonzero(mv >= 0)[0], mv[mv >= 0],
                        lambda i, m: f"game {ids[i]} ply {ply}: sampled move {m} is illegal")
            kept[rl_end:sl_start] = pos[rl_end:sl_start]
        t = lap("rules", t)
    if finish:
        from . import rollout
        fin = rollout.finish_games(pos, rl, seed, counters=move_counters(ids, MAX_TURNS), rules=rules, device=dev,
                                   komi=KOMI)
        score = fin.score.astype(np.float64)
        kept = kept.cpu().numpy() if rules == "device" else kept
        t = lap("finish", t)
    elif rules == "device":
        score = T.area_score(pos, KOMI)
        t = lap("score", t)
        score, kept = score.cpu().numpy().astype(np.float64), kept.cpu().numpy()
    else:
        score = L.area_score_host(pos, KOMI)
    out = r, hist.cpu().numpy(), kept, score
    lap("download", t)
    return out


def generate(sl, rl, games, batch, seed, device=None, rules="device", timing=None, finish=False):
    """Play `games` games (ids 0 .. games-1) in passes of `batch`; sl, rl: fp32 LeafEngines (policy weights, max_batch >=
    batch).  rules="device": bkt_play_moves and bkt_area_score; "host": the host rules of reinforce.play_games(rules=
    "host") (lockstep: features_batch, the upload, play_host, area_score_host), the reference the tests and the benchmark
    compare against.  timing: a dict that receives seconds per phase ('engine', 'sampler', 'rules', 'download', and
    'score' with the device rules); the phases are then separated by
    synchronisations, so pass it only to measure.  finish: the RL engine plays every game out after turn 90 and the
    score is the finished board's (phase 'finish' instead of 'score').  -> Generated."""
    L.check_rules(rules)
    if not 1 <= batch <= T.MAX_BATCH:
        raise ValueError(f"batch must be 1..{T.MAX_BATCH}, got {batch}")
    dev = torch.device("cuda", sl.device_id) if device is None else torch.device(device)
    G = int(games)
    out = Generated()
    out.r = np.zeros(G, np.int64)
    out.moves = np.full((G, MAX_TURNS), -1, np.int16)
    out.score = np.zeros(G, np.float64)
    out.kept = np.zeros(G, bool)
    rows, row_game = [], []
    for s in range(0, G, batch):
        ids = np.arange(s, min(s + batch, G), dtype=np.int64)
        order = ids[np.argsort(random_ply(ids, seed), kind="stable")]
        r, hist, kept, score = _pass(sl, rl, order, seed, dev, rules, timing, finish)
        out.r[order], out.moves[order] = r, hist
        out.score[order] = score
        ok = hist[np.arange(len(order)), r] >= 0       # a game stuck before or at r_g stays stuck: -1 at ply r_g
        out.kept[order] = ok
        sel = np.nonzero(ok)[0]
        sel = sel[np.argsort(order[sel])]
        boards, ko, last, turn = _record_fields(kept[sel])
        black_won = score[sel] > 0
        val = np.where((turn % 2 == 0) == black_won, 1, -1)
        rows += list(zip(boards, ko.tolist(), last.tolist(), turn.tolist(), val.tolist()))
        row_game.append(order[sel])
    out.rows = rows
    out.game = np.concatenate(row_game) if row_game else np.zeros(0, np.int64)
    return out


# ---- the command line -------------------------------------------------------------------------------------------------------
def _parse(argv):
    ap = argparse.ArgumentParser(description="Generate value-net training data from SL-then-RL policy games on the "
                                             "MI355X (the reference's bin/genvals.py)")
    ap.add_argument("-o", dest="o", metavar="PATH", required=True, help="output CSV (appended to)")
    ap.add_argument("-w", dest="w", metavar="POOL", default=None,
                    help="a pool of policy_<id>.pt / .bkw: SL = the lowest id, RL = the highest")
    ap.add_argument("--sl", default=None, help="SL policy (.pt or .bkw)")
    ap.add_argument("--rl", default=None, help="RL policy (.pt or .bkw)")
    ap.add_argument("-n", dest="n", metavar="N", type=int, default=1, help="number of games in thousands")
    ap.add_argument("--games", type=int, default=None, help="exact number of games (overrides -n)")
    ap.add_argument("--batch", type=int, default=4096, help="games per lock-step pass")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--finish", action="store_true",
                    help="the RL policy plays every game out after turn 90; the label comes from the finished board")
    args = ap.parse_args(argv)
    if args.w is None and args.sl is None and args.rl is None:
        ap.error("no policies: give -w POOL or --sl PATH --rl PATH")
    if args.w is not None and (args.sl is not None or args.rl is not None):
        ap.error("-w and --sl/--rl exclude each other")
    if args.w is None and (args.sl is None or args.rl is None):
        ap.error("--sl and --rl go together")
    if not 1 <= args.batch <= T.MAX_BATCH:
        ap.error(f"--batch must be 1..{T.MAX_BATCH}")
    args.games = args.n * 1000 if args.games is None else args.games
    if args.games < 1:
        ap.error("the number of games must be at least 1")
    if not (0 <= args.seed < 2 ** 64):
        ap.error("--seed must be an unsigned 64-bit integer")
    if args.w is not None:
        if not os.path.isdir(args.w):
            ap.error(f"-w {args.w}: not a directory")
        pool = R.policy_pool(args.w)
        if not pool:
            ap.error(f"-w {args.w}: no policy_<id>.pt or .bkw")
        args.sl, args.rl = pool[min(pool)], pool[max(pool)]
    return args


def main(argv=None):
    from .train import load_weights

    args = _parse(argv)
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    sl = R.policy_engine(load_weights(args.sl), args.device, args.batch)
    rl = R.policy_engine(load_weights(args.rl), args.device, args.batch)
    try:
        t0 = time.perf_counter()
        out = generate(sl, rl, args.games, args.batch, args.seed, dev, finish=args.finish)
        dt = time.perf_counter() - t0
    finally:
        sl.close()
        rl.close()
    write_rows(args.o, out.rows)
    print(json.dumps({"sl": args.sl, "rl": args.rl, "games": args.games, "rows": len(out.rows),
                      "dropped": int((~out.kept).sum()), "games_per_s": args.games / dt, "seconds": dt,
                      "out": args.o}), flush=True)


if __name__ == "__main__":
    main()

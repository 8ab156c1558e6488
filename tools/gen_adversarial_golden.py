#!/usr/bin/env python3
"""tests/golden/adversarial_boards.npz: the REFERENCE's answers on the hand-built corpus of tests/adversarial_boards.py.
Per corpus position: nnet.features' 27 planes, Game.get_liberties, Game.get_legal_moves, Game.score, and for each of the
81 points what Game.play_move does -- the outcome (played / ko / not_empty / suicide), the new ko point and the resulting
board, kept as the set of captured points.  Data only: the corpus in, arrays out.

A board record is go.Game(board=, ko=, last_move=, turn=) there as here.  A script record is its board played on with
play_move, get_liberties() before the first move and after every move (what features() does in a game), so that the
liberty cache has the history the record's has; a move the reference refuses is skipped, as the corpus skips it.

The densest random boards are left out when the file would pass 256 KB (they stay in the GPU corpus): `kept` names the
corpus rows the file holds.

    python tools/gen_adversarial_golden.py     # needs the reference checkout (BOKEGO_REFERENCE, default /root/reference)
"""
import os
import sys

REF = os.environ.get("BOKEGO_REFERENCE", "/root/reference")
if not os.path.isdir(os.path.join(REF, "bokego")):
    sys.exit(f"reference checkout not found at {REF}; set BOKEGO_REFERENCE")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REF, ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import bokego.go as rgo  # noqa: E402
import bokego.nnet as rnn  # noqa: E402

import adversarial_boards as A  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "adversarial_boards.npz")
LIMIT = 256 * 1024
OUTCOME = {None: 0, "ko": 1, "not_empty": 2, "suicide": 3}


def reference_game(C, origin):
    if origin.kind == "board":
        c = C.cases[origin.index]
        return rgo.Game(board=c.board, ko=c.ko, last_move=c.last_move, turn=c.turn)
    s = C.scripts[origin.index]
    g = rgo.Game(board=s.board, turn=s.turn)
    g.get_liberties()
    for mv in s.moves[:origin.ply]:
        try:
            g.play_move(mv)
        except rgo.IllegalMove:
            continue
        g.get_liberties()
    return g


def clone(g):
    h = rgo.Game(board=g.board, ko=g.ko, last_move=g.last_move, turn=g.turn)
    h._libs = None if g._libs is None else bytearray(g._libs)
    return h


def answers(g):
    planes = rnn.features(clone(g)).numpy().astype(np.uint8).reshape(27, 81)
    libs = np.array(clone(g).get_liberties(), np.uint8)
    legal = np.zeros(81, np.uint8)
    legal[clone(g).get_legal_moves()] = 1
    outcome, ko, captured = np.zeros(81, np.uint8), np.full(81, -1, np.int8), np.zeros((81, 81), bool)
    for m in range(81):
        h = clone(g)
        try:
            h.play_move(m)
        except rgo.IllegalMove as e:
            outcome[m] = OUTCOME[e.rule_type]
            assert h.board == g.board
            continue
        ko[m] = -1 if h.ko is None else h.ko
        want = g.board[:m] + "XO"[g.turn % 2] + g.board[m + 1:]
        captured[m] = [a != b for a, b in zip(want, h.board)]
        assert all(b == "." for a, b in zip(want, h.board) if a != b)
    return planes, libs, legal, np.float32(g.score()), outcome, ko, np.packbits(captured, axis=1)


def main():
    C = A.check_conditions()
    rows = list(range(len(C.names)))
    got = {i: answers(reference_game(C, C.origins[i])) for i in rows}
    dense = [f"dense{d}_" for d in reversed(A.DENSITIES)]
    while True:
        cols = [np.stack([got[i][k] for i in rows]) for k in range(7)]
        np.savez_compressed(OUT, kept=np.array(rows, np.int32), names=np.array([C.names[i] for i in rows]),
                            records=C.recs[rows], planes=cols[0], liberties=cols[1], legal=cols[2], score=cols[3],
                            outcome=cols[4], ko=cols[5], captured=cols[6])
        size = os.path.getsize(OUT)
        if size <= LIMIT or not dense:
            break
        drop = dense.pop(0)
        rows = [i for i in rows if not C.names[i].startswith(drop)]
    print(f"{len(rows)} of {len(C.names)} corpus positions, {size} bytes")


if __name__ == "__main__":
    main()

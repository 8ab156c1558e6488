"""Hand-built boards that no played game reaches, for every kernel that reads a Go board.  A plain helper
module, shared by test_adversarial_boards_cpu.py (the host rules against the reference's recorded answers, the Python
mirrors against the C functions) and test_gpu_adversarial_boards.py (every device entry point against the host rules), so
that both are held to the same records.  Nothing here needs a GPU, and nothing is read from a file.

The corpus (corpus()) is a list of named 192-byte bk_pos records of two kinds:

  board records   go.Game(board=, ko=, last_move=, turn=): the liberty cache is invalid, the first refresh recounts
                  every chain.  Every named board comes with black and with white to move (turn 0 and 1; also a turn
                  that no black-first game could have on that board), some with the last move a pass and some with a ko
                  set on a point that would otherwise be legal.
  script records  a named board played on with bk_pos_play (+ bk_pos_liberties after every move, as the device does): the
                  record after each accepted move, taken before that refresh, so that the cache is valid, holds the stale
                  counts the captures left behind, and a refresh is pending.

check_conditions() asserts, with a plain Python flood and the host library alone, that the boards have the properties they
were built for.  They are conditions, not measurements: a corpus that loses one fails on the CPU.
"""
import ctypes
from collections import namedtuple

import numpy as np

from bokego_amd import go

PASS = go.PASS
OFF_LIBS, OFF_VALID, OFF_KO, OFF_LAST, OFF_TURN = 81, 162, 164, 166, 172

Case = namedtuple("Case", "name board ko last_move turn")              # a board record
Script = namedtuple("Script", "name board turn moves")                 # moves: played in order; refused ones are skipped
Origin = namedtuple("Origin", "kind index ply")                        # ("board", case, 0) | ("script", script, plies played)
Corpus = namedtuple("Corpus", "names recs origins cases scripts")


def B(*rows):
    s = "".join(rows).replace(" ", "")
    assert len(s) == 81, len(s)
    return s


def swap(board):
    return board.translate(str.maketrans("XO", "OX"))


# ---- the boards ------------------------------------------------------------------------------------------------------------
# A one-stone-wide chain from the corner 0 to the centre 40: 49 stones, 48 flood rounds from either end; its complement is
# one empty corridor of 32 points from 9 to 48, 31 rounds from either end.
SPIRAL = B("X X X X X X X X X",
           ". . . . . . . . X",
           "X X X X X X X . X",
           "X . . . . . X . X",
           "X . X X X . X . X",
           "X . X . . . X . X",
           "X . X X X X X . X",
           "X . . . . . . . X",
           "X X X X X X X X X")
SPIRAL_ENDS, CORRIDOR_ENDS = (0, 40), (9, 48)
# the same corridor between two colours: the inner turns of the spiral are white
SPIRAL_TWO = "".join("O" if c == "X" and 2 <= i // 9 <= 6 and 2 <= i % 9 <= 6 else c for i, c in enumerate(SPIRAL))

# Eight white stones around the centre whose only liberty it is: black's move there is touched four times by one chain
RING = B(". . . . . . . . .",
         ". . . . . . . . .",
         ". . . X X X . . .",
         ". . X O O O X . .",
         ". . X O . O X . .",
         ". . X O O O X . .",
         ". . . X X X . . .",
         ". . . . . . . . .",
         ". . . . . . . . .")

# Four white chains of six stones whose only liberty is the centre; black everywhere else but in the corners
ARMS = B(". X X X X X X X .",
         "X O X X O O O O X",
         "X O X X O X X X X",
         "X O X X O X X X X",
         "X O O O . O O O X",
         "X X X X O X X O X",
         "X X X X O X X O X",
         "X O O O O X X O X",
         ". X X X X X X X .")

CAP80_CENTRE = "O" * 40 + "." + "O" * 40
CAP80_CORNER = "." + "O" * 80
# every stone without a liberty; black's move at the hole captures four single stones, white has no legal point
CHECKER = "".join("." if i == 40 else "XO"[(i // 9 + i % 9) % 2] for i in range(81))

KO_CENTRE = B(". . . . . . . . .",
              ". . . . . . . . .",
              ". . . . . . . . .",
              ". . . X O . . . .",
              ". . X O . O . . .",
              ". . . X O . . . .",
              ". . . . . . . . .",
              ". . . . . . . . .",
              ". . . . . . . . .")                                        # black 40 takes 39
KO_EDGE = B(". X O . O . . . .",
            ". . X O . . . . .", *["." * 9] * 7)                           # black 3 takes 2
KO_CORNER = B(". O X . . . . . .",
              "O X . . . . . . .", *["." * 9] * 7)                         # black 0 takes 1
KOS = {"ko_centre": (KO_CENTRE, 40, 39), "ko_edge": (KO_EDGE, 3, 2), "ko_corner": (KO_CORNER, 0, 1)}

# black 2 takes the single stones 1 and 3, every neighbour white: two stones, so no ko
TWO_SINGLES = B("X O . O X . . . .",
                ". X O X . . . . .", *["." * 9] * 7)
# black 2 joins two stones and has no liberty: a suicide of three
SUICIDE3 = B("X X . O . . . . .",
             "O O O . . . . . .", *["." * 9] * 7)
# black 2 (one liberty, 3), white 3 takes it (no ko: its own stones are beside it), black 2 again takes seven
SNAPBACK = B("X O . . O X . . .",
             "X O O O O X . . .",
             ". X X X X . . . .", *["." * 9] * 6)
# black 40 joins four chains (16 liberties afterwards); white's move there is suicide
JOIN4 = B(". . . . . . . . .",
          ". . . . . . . . .",
          ". . . . X . . . .",
          ". . . . X . . . .",
          ". . X X . X X . .",
          ". . . . X . . . .",
          ". . . . X . . . .",
          ". . . . . . . . .",
          ". . . . . . . . .")
# black 2 takes five stones and has no other liberty than the three captured points beside it
EYE_CAPTURE = B("X O . O X . . . .",
                "X O O O X . . . .",
                ". X X X . . . . .", *["." * 9] * 6)
# chains of 8 and of 7 liberties; black 42 has 10 liberties afterwards
LINES = B(". . . . . . . . .",
          ". . O O O . . . .",
          ". . . . . . . . .",
          ". . . . . . . . .",
          ". . . X X X . . .",
          ". . . . . . . . .",
          ". . . . . . . . .",
          ". . . . . . O O O",
          ". . . . . . . . .")
# black 0 takes the three stones 1, 9, 10, touched at two points (test_gpu_genvals.py's board)
DOUBLE = B(". O X . . . . . .",
           "O O X . . . . . .",
           "X X . . . . . . .", *["." * 9] * 6)

NAMED = [("spiral", SPIRAL), ("spiral_swapped", swap(SPIRAL)), ("spiral_two", SPIRAL_TWO), ("ring", RING), ("arms", ARMS),
         ("cap80_centre", CAP80_CENTRE), ("cap80_corner", CAP80_CORNER), ("checker", CHECKER), ("ko_centre", KO_CENTRE),
         ("ko_edge", KO_EDGE), ("ko_corner", KO_CORNER), ("two_singles", TWO_SINGLES), ("suicide3", SUICIDE3),
         ("snapback", SNAPBACK), ("join4", JOIN4), ("eye_capture", EYE_CAPTURE), ("lines", LINES), ("double", DOUBLE)]
NAMED += [(n + "_white", swap(b)) for n, b in NAMED[3:]]                  # the same shapes with the colours swapped

DENSITIES, DENSE_EACH = (0.5, 0.7, 0.85, 0.95), 40


def dense_boards():
    """40 seeded random boards at each density: chains without liberties among them, as bk_pos_from_board accepts."""
    rng = np.random.default_rng(3)
    out = []
    for d in DENSITIES:
        for k in range(DENSE_EACH):
            a, col = rng.random(81), rng.random(81) < 0.5
            out.append((f"dense{d}_{k}", "".join("." if a[i] > d else "XO"[int(col[i])] for i in range(81))))
    return out


def cases():
    out = []
    for name, b in NAMED + dense_boards():
        out += [Case(f"{name}/b", b, None, None, 0), Case(f"{name}/w", b, None, None, 1)]
    for name, b in NAMED[:8] + NAMED[14:18]:
        # the last move a pass; a turn whose parity the stones contradict (49 black stones and no white one at turn 5)
        out += [Case(f"{name}/pass_b", b, None, PASS, 2), Case(f"{name}/pass_w", b, None, PASS, 3),
                Case(f"{name}/odd", b, None, None, 5), Case(f"{name}/even", b, None, None, 6)]
    # a ko set on a point that would otherwise be legal, with a last move beside it; and on the one legal point
    for name, b, ko, last in (("ring", RING, 40, 31), ("arms", ARMS, 40, 31), ("join4", JOIN4, 40, 22), ("lines", LINES, 42, 41),
                              ("cap80_centre", CAP80_CENTRE, 40, 39), ("checker", CHECKER, 40, 39), ("spiral", SPIRAL, 48, 49),
                              ("eye_capture", EYE_CAPTURE, 2, 1), ("two_singles", TWO_SINGLES, 2, 11)):
        last = last if b[last] != "." else None
        out += [Case(f"{name}/ko_b", b, ko, last, 0), Case(f"{name}/ko_w", b, ko, last, 1)]
    return out


def scripts():
    """Move lists for bk_pos_play.  A move the rules refuse leaves the record alone and the script goes on; which are
    refused, and why, is check_conditions' business."""
    out = []
    for name, (b, take, ko) in KOS.items():
        # the capture, the immediate retake (refused), a move elsewhere each, the retake (a ko again), and back (refused)
        out.append(Script(name, b, 0, (take, ko, 80, 70, ko, take, 60, 61, take)))
        out.append(Script(name + "_white", swap(b), 1, (take, ko, 80, 70, ko, take, PASS, PASS, take)))
    out.append(Script("snapback", SNAPBACK, 0, (2, 3, 2, 3, 12)))
    # onto a captured point whose stale count is not zero (the second refresh is skipped), then beside one
    out.append(Script("double", DOUBLE, 0, (0, 10, 9, 1, 40, 1)))
    out.append(Script("ring", RING, 0, (40, 30, 31, 39, 48, 30, 39, 32)))
    out.append(Script("arms", ARMS, 0, (40, 31, 39, 41, 49, 22, 0, 13)))
    out.append(Script("cap80_centre", CAP80_CENTRE, 0, (40, 39, 41, 31, 49, 30)))
    out.append(Script("cap80_corner", CAP80_CORNER, 0, (0, 1, 9, 10, 2)))
    out.append(Script("checker", CHECKER, 0, (40, 31, 39, 41, 49, 31)))
    out.append(Script("eye_capture", EYE_CAPTURE, 0, (2, 1, 3, 11, 10, 1)))
    out.append(Script("two_singles", TWO_SINGLES, 0, (2, 1, 3, 1)))
    out.append(Script("join4", JOIN4, 0, (40, 30, 32, 48, 50)))
    out.append(Script("spiral_two", SPIRAL_TWO, 1, (48, 9, 47, 10)))
    return out


# ---- records ---------------------------------------------------------------------------------------------------------------
_PP = ctypes.POINTER(go.Pos)
_cache = {}


def board_record(c):
    g = go.Game(board=c.board, ko=c.ko, last_move=c.last_move, turn=c.turn)
    return np.frombuffer(bytes(g._pos), np.uint8).copy()


def _ptr(rec):
    return ctypes.cast(rec.ctypes.data, _PP)


def play(rec, move, refresh=True):
    """bk_pos_play on a record in place -> (status, the record as bk_pos_play left it); refresh: bk_pos_liberties after
    an accepted move, which is what every device entry point does before it returns."""
    rc = go.golib().bk_pos_play(_ptr(rec), int(move))
    left = rec.copy()
    if rc == 0 and refresh:
        go.golib().bk_pos_liberties(_ptr(rec), (ctypes.c_uint8 * 81)())
    return rc, left


def script_records(s):
    """-> [(plies played, status of that move, the record before the pending refresh)] for the accepted moves of s."""
    rec = board_record(Case(s.name, s.board, None, None, s.turn))
    out = []
    for k, mv in enumerate(s.moves):
        rc, left = play(rec, mv)
        if rc == 0:
            out.append((k + 1, left))
    return out


def corpus():
    """-> Corpus(names, recs uint8 [n,192] (read only), origins, cases, scripts)."""
    if "corpus" not in _cache:
        cs, ss = cases(), scripts()
        names, recs, origins = [], [], []
        for i, c in enumerate(cs):
            names.append(c.name)
            recs.append(board_record(c))
            origins.append(Origin("board", i, 0))
        for i, s in enumerate(ss):
            for ply, rec in script_records(s):
                names.append(f"{s.name}/script{ply}")
                recs.append(rec)
                origins.append(Origin("script", i, ply))
        recs = np.ascontiguousarray(np.stack(recs))
        recs.setflags(write=False)
        _cache["corpus"] = Corpus(names, recs, origins, cs, ss)
    return _cache["corpus"]


def index(name):
    return corpus().names.index(name)


def refreshed(recs):
    """Copies of the records with bk_pos_liberties applied: what a caller hands to an entry point that reads the cache
    and does not refresh it (the feature encoder behind bk_encode_positions / bk_submit_positions)."""
    out = np.array(recs, np.uint8, order="C")
    tmp = (ctypes.c_uint8 * 81)()
    for i in range(len(out)):
        go.golib().bk_pos_liberties(_ptr(out[i]), tmp)
    return out


def rolled(recs):
    """Three batches in which every record sits in each of the three seats of a workgroup: the records rolled by 0, 1, 2."""
    return [np.ascontiguousarray(np.roll(recs, k, axis=0)) for k in range(3)]


def small_batches(recs, rows=(1, 2, 3, 4)):
    """Batches of 1, 2, 3 and 4 rows that walk through all records: -> [(start indices..., batch)]; every record is in at
    least one batch of every size, so also alone in a workgroup and in the last, partial one."""
    n = len(recs)
    for b in rows:
        for lo in range(0, n, b):
            idx = np.arange(lo, lo + b) % n
            yield idx, np.ascontiguousarray(recs[idx])


# ---- the conditions ----------------------------------------------------------------------------------------------------------
def flood(board, s):
    """Plain breadth-first flood of the points of board[s]'s kind from s -> (rounds until nothing is added, the region)."""
    seen, frontier, rounds = {s}, [s], 0
    while frontier:
        nxt = []
        for p in frontier:
            for t in go.NEIGHBORS[p]:
                if board[t] == board[s] and t not in seen:
                    seen.add(t)
                    nxt.append(t)
        frontier = nxt
        rounds += bool(nxt)
    return rounds, seen


def legal_points(rec):
    buf = (ctypes.c_uint8 * 81)()
    go.golib().bk_pos_legal_moves(_ptr(np.array(rec)), buf)
    return [s for s in range(81) if buf[s]]


def playable_points(rec):
    rec = np.array(rec)
    mover = 2 if rec[OFF_TURN] & 1 else 1
    return [s for s in legal_points(rec) if go.golib().bk_pos_possible_eye(_ptr(rec), s) != mover]


def _planes(rec):
    out = np.empty((27, 81), np.uint8)
    go.golib().bk_pos_features_u8(_ptr(np.array(rec)), out.ctypes.data, 0)
    return out


def _captures(board, turn, move):
    """Play move on the board record -> (status, stones captured, ko afterwards, the record)."""
    rec = board_record(Case("", board, None, None, turn))
    rc, _ = play(rec, move)
    after = rec[:81].view(np.int8)
    opp = "XO"[1 - (turn & 1)]
    gone = sum(1 for s in range(81) if board[s] == opp and after[s] == 0)
    return rc, gone, int(rec[OFF_KO:OFF_KO + 2].view(np.int16)[0]), rec


def check_conditions():
    C = corpus()
    assert len(C.names) == len(set(C.names)) == len(C.recs)
    kinds = [o.kind for o in C.origins]
    assert kinds.count("board") == len(C.cases) and kinds.count("script") >= 60
    assert (C.recs[[k == "board" for k in kinds], OFF_VALID] == 0).all()
    assert (C.recs[[k == "script" for k in kinds], OFF_VALID] == 1).all()
    turns = C.recs[:, OFF_TURN]
    assert (turns & 1).sum() >= len(C.recs) // 3 and (~turns & 1).sum() >= len(C.recs) // 3
    last = np.ascontiguousarray(C.recs[:, OFF_LAST:OFF_LAST + 2]).view(np.int16)[:, 0]
    ko = np.ascontiguousarray(C.recs[:, OFF_KO:OFF_KO + 2]).view(np.int16)[:, 0]
    assert (last == PASS).sum() >= 24 and (ko >= 0).sum() >= 24
    assert len(dense_boards()) == 160

    # the spiral: flood depth of the chain and of the corridor, from either end
    for b in (SPIRAL, swap(SPIRAL)):
        for end in SPIRAL_ENDS:
            rounds, chain = flood(b, end)
            assert rounds >= 48 and len(chain) == 49, (rounds, len(chain))
    for b in (SPIRAL, SPIRAL_TWO):
        for end in CORRIDOR_ENDS:
            rounds, region = flood(b, end)
            assert b[end] == "." and rounds >= 31 and len(region) == 32, (rounds, len(region))
    touch = lambda b: {b[t] for s in flood(b, 9)[1] for t in go.NEIGHBORS[s]} - {"."}   # noqa: E731
    assert touch(SPIRAL) == {"X"} and touch(SPIRAL_TWO) == {"X", "O"}

    # the ring: 8 stones, the move touched four times by one chain
    f = _planes(C.recs[index("ring/b")])
    assert f[5, 40] == 1 and f[13:20, 40].tolist() == [0, 0, 0, 4, 0, 0, 0] and f[20:27, 40].tolist() == [0, 0, 0, 0, 0, 0, 7]
    assert _captures(RING, 0, 40)[:3] == (0, 8, -1)
    assert len(flood(RING, 30)[1]) == 8 and all(RING[t] == "O" for t in go.NEIGHBORS[40])
    # four arms: four separate chains of six, 24 stones in one move
    chains = {frozenset(flood(ARMS, t)[1]) for t in go.NEIGHBORS[40]}
    assert len(chains) == 4 and all(len(c) == 6 for c in chains)
    assert _captures(ARMS, 0, 40)[:3] == (0, 24, -1) and _captures(ARMS, 1, 40)[0] == -13
    assert _planes(C.recs[index("arms/b")])[20:27, 40].tolist() == [0, 0, 0, 0, 0, 0, 7]
    # 80 stones: one legal point for black, none for white
    for name, b, at in (("cap80_centre", CAP80_CENTRE, 40), ("cap80_corner", CAP80_CORNER, 0)):
        assert _captures(b, 0, at)[:3] == (0, 80, -1) and _captures(b, 1, at)[0] == -13
        assert legal_points(C.recs[index(name + "/b")]) == [at] and playable_points(C.recs[index(name + "/b")]) == [at]
        assert legal_points(C.recs[index(name + "/w")]) == [] and playable_points(C.recs[index(name + "/w")]) == []
        assert legal_points(C.recs[index(name + "_white/w")]) == [at] and legal_points(C.recs[index(name + "_white/b")]) == []
    # the checkerboard: four single stones, every neighbour white, and no ko
    assert all(CHECKER[t] == "O" and len(flood(CHECKER, t)[1]) == 1 for t in go.NEIGHBORS[40])
    assert _captures(CHECKER, 0, 40)[:3] == (0, 4, -1) and _captures(CHECKER, 1, 40)[0] == -13
    assert legal_points(C.recs[index("checker/b")]) == [40] and legal_points(C.recs[index("checker/w")]) == []
    assert _planes(C.recs[index("checker/b")])[20:27, 40].tolist() == [0, 0, 0, 4, 0, 0, 0]
    # the kos: one stone, the retake refused at once and allowed after a move elsewhere
    for name, (b, take, point) in KOS.items():
        rc, gone, k, rec = _captures(b, 0, take)
        assert (rc, gone, k) == (0, 1, point), (name, rc, gone, k)
        assert play(rec.copy(), point)[0] == -11
        for mv in (80, 70):
            assert play(rec, mv)[0] == 0
        assert play(rec, point)[0] == 0 and int(rec[OFF_KO:OFF_KO + 2].view(np.int16)[0]) == take
        assert index(f"{name}/script1") and f"{name}/script2" not in C.names and f"{name}/script5" in C.names
    assert KOS["ko_edge"][1] // 9 == 0 and KOS["ko_corner"][1] == 0 and KOS["ko_centre"][1] == 40
    # two single stones at once: no ko although every neighbour is white
    assert all(TWO_SINGLES[t] == "O" for t in go.NEIGHBORS[2]) and _captures(TWO_SINGLES, 0, 2)[:3] == (0, 2, -1)
    # suicide of three; the snapback; four chains joined; liberties from the captures alone
    assert _captures(SUICIDE3, 0, 2)[0] == -13 and len(flood(SUICIDE3, 0)[1]) == 2
    rec = board_record(Case("", SNAPBACK, None, None, 0))
    assert [play(rec, m)[0] for m in (2, 3, 2)] == [0, 0, 0] and (rec[:81] == 2).sum() == 0 and rec[OFF_KO + 1] == 255
    assert len({frozenset(flood(JOIN4, t)[1]) for t in go.NEIGHBORS[40]}) == 4
    f = _planes(C.recs[index("join4/b")])
    assert f[19, 40] == 7 and f[5, 40] == 1 and _planes(C.recs[index("join4/w")])[5, 40] == 0
    rc, gone, k, rec = _captures(EYE_CAPTURE, 0, 2)
    assert (rc, gone, k) == (0, 5, -1) and all(EYE_CAPTURE[t] == "O" for t in go.NEIGHBORS[2])
    assert _planes(C.recs[index("eye_capture/b")])[13:20, 2].tolist() == [0, 0, 3, 0, 0, 0, 0]
    # the clips: chains of more than six liberties (plane 12), a move with more than six afterwards (plane 19)
    f = _planes(C.recs[index("lines/b")])
    assert f[12, 40] == 7 and f[12, 11] == 7 and f[19, 42] == 7 and f[6:12, 40].sum() == 0
    # after a capture: a stone onto a captured point whose stale count is not zero, and one beside it
    rec = board_record(Case("", DOUBLE, None, None, 0))
    assert play(rec, 0)[0] == 0 and rec[:81][[1, 9, 10]].tolist() == [0, 0, 0] and rec[OFF_LIBS + 10] != 0
    assert play(rec, 10)[0] == 0 and rec[OFF_LIBS + 10] == 1, "the stale count must survive: the refresh is skipped"
    stale = C.recs[index("ring/script1")]
    assert stale[OFF_VALID] == 1 and (stale[OFF_LIBS:OFF_LIBS + 81][stale[:81] == 0] != 0).sum() == 8
    stale = C.recs[index("cap80_centre/script1")]
    assert (stale[OFF_LIBS:OFF_LIBS + 81][stale[:81] == 0] != 0).sum() == 80
    # dense boards hold chains without a liberty, which no game reaches
    dead = 0
    for name, b in dense_boards()[120:]:
        libs = np.array(go.Game(board=b).get_liberties())
        dead += int(((libs == 0) & (np.array(list(b)) != ".")).any())
    assert dead >= 30, dead
    return C

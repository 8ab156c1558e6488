"""CPU: what the playout drivers share (bokego_amd/lockstep.py) -- the fields of a record read from numpy and from a
tensor, the one builder of the Philox counter layouts, and engine_logits' calls."""
import numpy as np
import torch

from bokego_amd import genvals, go
from bokego_amd import lockstep as L
from bokego_amd import rollout as RO

# black at 11 captures the white stone at 10 and stands in atari there itself: a ko at 10
KO_BOARD = ".XO......" + "XO.O....." + ".XO......" + "........." * 6


def _records():
    """An empty board, a record after a move that sets a ko, a record after a pass -> (games, uint8 [3,192])."""
    ko = go.Game(KO_BOARD)
    ko.play_move(11)
    passed = go.Game()
    passed.play_pass()
    games = [go.Game(), ko, passed]
    return games, np.stack([np.frombuffer(bytes(g._pos), np.uint8) for g in games])


def test_record_fields_from_numpy_and_from_a_tensor():
    games, recs = _records()
    assert games[1]._pos.ko == 10 and games[2]._pos.last_move == go.PASS and games[1]._pos.hash >> 32
    tens = torch.from_numpy(recs.copy())
    for f, name, dtype in ((L.record_ko, "ko", np.int16), (L.record_last_move, "last_move", np.int16),
                           (L.record_turns, "turn", np.int32)):
        a, t = f(recs), f(tens)
        assert isinstance(a, np.ndarray) and isinstance(t, torch.Tensor) and t.device == tens.device
        assert a.dtype == dtype == t.numpy().dtype and a.shape == (3,) and np.array_equal(a, t.numpy())
        assert a.tolist() == [getattr(g._pos, name) for g in games], name
    a, t = L.record_hash_words(recs), L.record_hash_words(tens)
    assert a.dtype == np.int32 == t.numpy().dtype and a.shape == (3, 2) and np.array_equal(a, t.numpy())
    assert a.view(np.uint32).tolist() == [[g._pos.hash & 0xFFFFFFFF, g._pos.hash >> 32] for g in games]
    assert L.black_to_move(recs).tolist() == L.black_to_move(tens).tolist() == [True, False, False]
    assert np.array_equal(L.record_turns(recs[1:2]), [1]) and L.record_turns(recs[1:2]).base is None      # a copy
    assert np.array_equal(recs, tens.numpy())                        # nothing was written


def test_the_counter_builder_gives_the_literal_words_of_all_four_layouts():
    big = 2 ** 32 + 7                                                # the smallest kind of id whose high word is not zero
    ids = np.array([big, 0], np.uint64)
    c = genvals.move_counters(ids, 17)
    assert c.dtype == np.int32 and c.view(np.uint32).tolist() == [[7, 17, 1, 0], [0, 17, 0, 0]]
    c = L.game_counters(ids, 0, L.STREAM_R)                          # genvals.random_ply's draw
    assert c.dtype == np.int32 and c.view(np.uint32).tolist() == [[7, 0, 1, 1], [0, 0, 0, 1]]
    u = L.uniform(L.philox4x32_10(c.view(np.uint32), L.seed_key(99))[:, 0])
    assert genvals.random_ply(ids, 99).tolist() == (70 + np.floor(20 * u)).astype(np.int64).tolist()
    c = L.game_counters(ids, [41, 0], L.STREAM_ROLLOUT)              # rollout.default_counters with g = the ids
    assert c.view(np.uint32).tolist() == [[7, 41, 1, 2], [0, 0, 0, 2]]
    assert RO.default_counters(2, [0, 41]).view(np.uint32).tolist() == [[0, 0, 0, 2], [1, 41, 0, 2]]
    assert RO.default_counters(1, [-1]).view(np.uint32).tolist() == [[0, 0xFFFFFFFF, 0, 2]]
    recs = _records()[1][:2].copy()                                  # rollout.value_counters: g = the record's hash
    recs[:, L.OFF_HASH:] = np.array([big, 0], np.uint64).view(np.uint8).reshape(2, 8)
    c = RO.value_counters(recs, 3)
    assert c.dtype == np.int32 and c.shape == (6, 4)
    assert c.view(np.uint32).tolist() == [[7, 0, 1, 3], [7, 0, 1, 7], [7, 0, 1, 11], [0, 0, 0, 3], [0, 0, 0, 7], [0, 0, 0, 11]]
    d = L.value_counters_device(torch.from_numpy(recs), 3)           # the sibling that builds them where the records are
    assert d.dtype == torch.int32 and np.array_equal(d.numpy(), c)
    assert (L.STREAM_MOVE, L.STREAM_R, L.STREAM_ROLLOUT, L.STREAM_VALUE) == (0, 1, 2, 3)


class StubEngine:
    """eval_device returns, as 'logits', the first plane value of each row in 81 columns, and records its batch sizes."""

    def __init__(self, max_batch):
        self.max_batch, self.calls = max_batch, []

    def eval_device(self, planes, logits, probs, value):
        assert logits and not probs and not value and 1 <= len(planes) <= self.max_batch
        self.calls.append(len(planes))
        self.last = planes.reshape(len(planes), -1)[:, :1].float().repeat(1, 81)
        return {"logits": self.last}


def test_engine_logits_splits_by_max_batch_and_skips_empty_slices():
    planes = torch.arange(12, dtype=torch.uint8).reshape(12, 1, 1, 1).repeat(1, 27, 9, 9)
    a, b, c = StubEngine(4), StubEngine(4), StubEngine(4)
    out = L.engine_logits([(a, planes[:0]), (b, planes[:3]), (c, planes[3:])])
    assert (a.calls, b.calls, c.calls) == ([], [3], [4, 4, 1])
    assert out.shape == (12, 81) and out[:, 0].tolist() == list(range(12)) and out[:, 80].tolist() == list(range(12))
    one = StubEngine(4)
    part = planes[5:8]
    out = L.engine_logits([(one, part), (a, planes[:0])])            # one part: the engine's own tensor, no cat
    assert one.calls == [3] and a.calls == [] and out is one.last and out[:, 0].tolist() == [5, 6, 7]

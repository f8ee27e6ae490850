"""The global numpy stream's bookkeeping behind the PPO minibatch orders
(population/perms.py, ShuffleStream): host only, no device.  P = 3, S = 16,
E = 4 unless a case says otherwise."""

from types import SimpleNamespace

import numpy as np
import pytest

from agilerl_amd.population.perms import ShuffleStream
from agilerl_amd.rng import numpy_shuffle_perms

P, S, E = 3, 16, 4


def _values(P=P, global_P=None, agent_offset=0, target_kl=None):
    """The population values the bookkeeping reads when it draws."""
    global_P = P if global_P is None else global_P
    return SimpleNamespace(P=P, S=S, update_epochs=E, agent_epochs=[E] * P, heterogeneous=False, global_P=global_P,
                           agent_offset=agent_offset, global_epochs=[E] * global_P, perm_source="numpy",
                           target_kl=target_kl)


def _same_state(a, b) -> bool:
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _state():
    return np.random.get_state(legacy=True)


def test_draw_then_discard_restores_the_stream():
    book = ShuffleStream(_values())
    np.random.seed(5)
    before = _state()
    ahead = np.empty((E, P, S), dtype=np.int64)
    state = book.fill(ahead)
    assert not _same_state(_state(), before)
    book.rewind(state)
    assert _same_state(_state(), before)
    again = np.empty_like(ahead)
    book.fill(again)
    assert np.array_equal(again, ahead)
    assert np.array_equal(np.sort(again, axis=-1), np.broadcast_to(np.arange(S), (E, P, S)))


def test_target_kl_correction_advances_by_the_epochs_run():
    book = ShuffleStream(_values(target_kl=0.01))
    out = np.empty((E, P, S), dtype=np.int64)
    np.random.seed(11)
    book.drawn_state = book.fill(out)
    book.report([4, 2, 1])
    book.settle()
    got = _state()
    np.random.seed(11)
    numpy_shuffle_perms(1, 7, S)
    assert _same_state(got, _state())

    # every agent ran all its epochs: the stream stays where the draw left it
    np.random.seed(11)
    book.drawn_state = book.fill(out)
    drawn = _state()
    book.report([4, 4, 4])
    book.settle()
    assert _same_state(_state(), drawn)
    np.random.seed(11)
    numpy_shuffle_perms(P, E, S)
    assert _same_state(_state(), drawn)


def test_generation_block_rows_are_served_in_order():
    book = ShuffleStream(_values(target_kl=0.01))
    np.random.seed(3)
    block = numpy_shuffle_perms(2 * P, E, S).reshape(E, 2, P, S).transpose(1, 0, 2, 3).copy()  # [K = 2, E, P, S]
    before = _state()
    book.set_block(block)
    out = np.empty((E, P, S), dtype=np.int64)
    assert book.fill(out) is None and np.array_equal(out, block[0])
    book.report([4, 2, 1])  # kept for the engine, which re-syncs the stream after the generation
    # a row taken ahead and handed back is served again as the same row
    assert book.fill(out) is None and np.array_equal(out, block[1])
    book.give_back_row()
    assert not book.exhausted
    assert book.fill(out) is None and np.array_equal(out, block[1])
    assert book.exhausted
    book.report([4, 4, 4])
    assert book.generation_epochs_run() == [[4, 2, 1], [4, 4, 4]] and book.pending is None
    assert _same_state(_state(), before)
    with pytest.raises(RuntimeError, match="more learns than the generation's shuffles were drawn for"):
        book.fill(out)
    assert _same_state(_state(), before)

    with pytest.raises(ValueError, match="generation shuffles"):
        book.set_block(block[:, :, :2])
    book.set_block(None)
    assert book.generation_epochs_run() == []
    assert book.fill(out) is not None  # a per-learn draw from the global stream again
    np.random.set_state(before)
    assert np.array_equal(out, numpy_shuffle_perms(P, E, S))


def test_sharded_draw_is_a_slice_of_the_whole_population():
    np.random.seed(21)
    whole = np.empty((E, 4, S), dtype=np.int64)
    ShuffleStream(_values(P=4)).fill(whole)
    after_whole = _state()
    np.random.seed(21)
    shard = np.empty((E, 2, S), dtype=np.int64)
    ShuffleStream(_values(P=2, global_P=4, agent_offset=1)).fill(shard)
    assert _same_state(_state(), after_whole)
    assert np.array_equal(shard, whole[:, 1:3])

"""The slot bookkeeping of a streaming decode session (avsr_amd/stream_slots.py) on the CPU: a
scripted stream through the same admit / step / finish loop the session runs, without a search."""
import pytest

from avsr_amd import stream_slots as SS


def _scripted_stream(book, frames, steps_needed):
    """DecodeSession.run's loop with the search replaced by a script: input i needs
    steps_needed[i] steps once admitted. Yields (index, result) in completion order and records
    the slot history in book."""
    inputs = iter(enumerate(frames))
    left, more = {}, True
    while True:
        while more and book.free_slot() is not None:
            nxt = next(inputs, None)
            if nxt is None:
                more = False
                break
            i, T = nxt
            if not book.fits(T):
                yield book.bypass(i), ("alone", i)
                continue
            left[book.admit(i, T)] = steps_needed[i]
        busy = book.busy()
        if not busy:
            return
        for slot in sorted(busy):
            left[slot] -= 1
            if left[slot] == 0:
                yield book.finish(slot), ("slot", slot, busy[slot])


def test_admission_follows_input_order_and_every_result_comes_once():
    """S = 2, five inputs finishing in the scripted order 1, 0, 3, 2, 4"""
    book = SS.SlotBook(2, 3, 100)
    steps = [5, 2, 6, 1, 3]
    out = list(_scripted_stream(book, [10, 20, 30, 40, 50], steps))
    assert [i for i, _ in book.admitted] == [0, 1, 2, 3, 4]
    # 1 ends at step 2 (slot 1 <- 2), 0 at step 5 (slot 0 <- 3), 3 at step 6 (slot 0 <- 4), 2 at 8, 4 at 9
    assert book.admitted == [(0, 0), (1, 1), (2, 1), (3, 0), (4, 0)]
    assert [i for i, _ in out] == book.completed == [1, 0, 3, 2, 4]
    assert sorted(i for i, _ in out) == list(range(5))
    assert all(r == ("slot", s, i) for (i, r), s in zip(out, [1, 0, 0, 1, 0]))
    assert book.busy() == {} and book.free_slot() == 0


def test_stream_order_equals_input_order():
    book = SS.SlotBook(2, 3, 100)
    out = list(_scripted_stream(book, [10] * 5, [5, 2, 6, 1, 3]))
    assert [i for i, _ in out] != list(range(5))
    assert [r[2] for r in SS.in_input_order(out, 5)] == list(range(5))
    with pytest.raises(RuntimeError):
        SS.in_input_order(out + out[:1], 5)          # delivered twice
    with pytest.raises(RuntimeError):
        SS.in_input_order(out[:-1], 5)               # one missing


def test_oversize_input_goes_to_the_fallback():
    book = SS.SlotBook(2, 3, 25)
    out = list(_scripted_stream(book, [10, 26, 25, 40, 3], [4, 9, 2, 9, 1]))
    assert dict(out)[1] == ("alone", 1) and dict(out)[3] == ("alone", 3)
    assert [i for i, _ in book.admitted] == [0, 2, 4]          # the oversize ones never take a slot
    assert [i for i, _ in out] == [1, 2, 3, 4, 0]              # delivered when the stream reaches them
    assert sorted(book.completed) == list(range(5))
    with pytest.raises(SS.CapacityError):
        book.admit(9, 26)
    with pytest.raises(SS.CapacityError):
        book.admit(9, 0)


def test_capacity_rules():
    with pytest.raises(ValueError):
        SS.SlotBook(13, 5, 375)                      # 65 rows
    with pytest.raises(ValueError):
        SS.check_geometry(22, 3)
    SS.check_geometry(12, 5)
    SS.check_geometry(64, 1)
    assert [SS.default_slots(b) for b in (1, 3, 5, 8, 10, 40)] == [8, 8, 8, 8, 6, 1]
    book = SS.SlotBook(2, 1, 10)
    book.admit(0, 5)
    book.admit(1, 5)
    with pytest.raises(RuntimeError):
        book.admit(2, 5)                             # no free slot
    assert book.finish(0) == 0
    with pytest.raises(RuntimeError):
        book.finish(0)                               # empty slot
    with pytest.raises(RuntimeError):
        book.admit(1, 5)                             # an index enters once

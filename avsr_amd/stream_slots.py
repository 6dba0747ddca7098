"""Slot bookkeeping of a streaming decode session (avsr_amd.decode.DecodeSession): which input
sits in which of the fixed utterance slots, in which order inputs were admitted and finished, and
the capacity rules. Plain Python (no torch, no GPU), so the host logic is testable on its own."""

ROW_LIMIT = 64          # rows of the few-row GEMM (ops.py, M <= 64): the kernel whose rows are batch-invariant


def default_slots(beam):
    """slots of a session when the caller names none: up to 8 utterances within the row limit"""
    return max(1, min(8, ROW_LIMIT // beam))


def check_geometry(slots, beam):
    """slots x beam rows must fit the few-row GEMM"""
    if slots < 1 or beam < 1:
        raise ValueError(f"slots = {slots}, beam = {beam}: both must be at least 1")
    if slots * beam > ROW_LIMIT:
        raise ValueError(f"slots * beam = {slots} * {beam} = {slots * beam} rows exceed the few-row GEMM's "
                         f"{ROW_LIMIT}-row limit: at beam {beam} a session holds at most {ROW_LIMIT // beam} slots")


class CapacityError(ValueError):
    """an input that does not fit a slot (more frames than the session's max_frames)"""


class SlotBook:
    """`slots` utterance slots of `max_frames` frames each. Inputs are identified by their index
    in the stream; an input is admitted into the lowest free slot, finished once, and an oversize
    input (routed to the one-utterance search by the session) is recorded with `bypass`."""

    def __init__(self, slots, beam, max_frames):
        check_geometry(slots, beam)
        if max_frames < 1:
            raise ValueError(f"max_frames = {max_frames}")
        self.slots, self.beam, self.max_frames = slots, beam, max_frames
        self._slot_of = {}            # input index -> slot, while it is being decoded
        self._index_in = [None] * slots
        self.admitted = []            # (index, slot) in admission order
        self.completed = []           # input indices in completion order (bypassed ones included)
        self._seen = set()

    def fits(self, frames):
        return 1 <= frames <= self.max_frames

    def free_slot(self):
        for s, i in enumerate(self._index_in):
            if i is None:
                return s
        return None

    def busy(self):
        """{slot: input index} of the slots that hold an utterance"""
        return {s: i for s, i in enumerate(self._index_in) if i is not None}

    def _new(self, index):
        if index in self._seen:
            raise RuntimeError(f"input {index} entered the stream twice")
        self._seen.add(index)

    def admit(self, index, frames):
        if not self.fits(frames):
            raise CapacityError(f"input {index}: {frames} frames do not fit a slot of {self.max_frames}")
        s = self.free_slot()
        if s is None:
            raise RuntimeError("no free slot")
        self._new(index)
        self._index_in[s] = index
        self._slot_of[index] = s
        self.admitted.append((index, s))
        return s

    def bypass(self, index):
        """an input decoded outside the slots (oversize): delivered at once"""
        self._new(index)
        self.completed.append(index)
        return index

    def finish(self, slot):
        index = self._index_in[slot]
        if index is None:
            raise RuntimeError(f"slot {slot} holds no utterance")
        self._index_in[slot] = None
        del self._slot_of[index]
        self.completed.append(index)
        return index


def in_input_order(pairs, n=None):
    """[(index, result), ...] in completion order -> results in input order; every index of
    range(n) exactly once"""
    out = {}
    for i, r in pairs:
        if i in out:
            raise RuntimeError(f"input {i} delivered twice")
        out[i] = r
    n = len(out) if n is None else n
    if sorted(out) != list(range(n)):
        raise RuntimeError(f"results for inputs {sorted(out)} of {n}")
    return [out[i] for i in range(n)]

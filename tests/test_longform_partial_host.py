"""The host side of partial long-form alignment (avsr_amd.longform): segments() and uncovered() on
hand-built PartialAlignments, gap_flags, and the argument errors of align_partial, which are
raised before the device is touched (the model stand-in here has no engine)."""
import numpy as np
import pytest
import torch

from avsr_amd import longform
from avsr_amd.align import TokenSpan

V = 12
TOKENS = ["<blank>"] + ["▁w%d" % i for i in range(1, V - 1)] + ["<eos>"]        # every piece is a word


def _partial(T, spans, gaps, seed=0):
    """spans: (token, start, end); gaps: [start, end) runs; ali and frame_logp made to match"""
    ali = np.zeros(T, np.int32)
    for k, a, b in spans:
        ali[a:b] = k
    for a, b in gaps:
        assert (ali[a:b] == 0).all()
        ali[a:b] = -2
    flp = -np.random.Generator(np.random.PCG64(seed)).random(T).astype(np.float32)
    return longform.PartialAlignment([TokenSpan(*s) for s in spans], float(flp.sum()), flp, [list(g) for g in gaps],
                                     ali)


def _no_gap_frames(segs, p):
    for s in segs:
        assert not (p.ali[s.start:s.end] == -2).any(), s


def _every_token_once(segs, p):
    assert [t for s in segs for t in s.tokens] == [sp.token for sp in p.spans]
    assert [s.first for s in segs] == [0] + [s.last + 1 for s in segs[:-1]] and segs[-1].last == len(p.spans) - 1
    assert all(a.end <= b.start for a, b in zip(segs, segs[1:]))


def test_forced_cut_at_a_gap_in_a_short_pause():
    """pauses of 20, 6 and 20 frames; the gap run sits in the 6-frame one. Everything fits in
    max_frames, so without the gap there is one clip; with it there are two, cut at the gap"""
    spans = [(1, 10, 20), (2, 40, 50), (3, 56, 66), (4, 86, 96)]
    p = _partial(110, spans, [(51, 55)])
    segs = longform.segments(p, TOKENS, max_frames=375)
    assert [(s.first, s.last) for s in segs] == [(0, 1), (2, 3)]
    assert segs[0].end <= 51 and segs[1].start >= 55
    _no_gap_frames(segs, p)
    _every_token_once(segs, p)
    whole = longform.segments(longform.LongAlignment(p.spans, p.score, p.frame_logp), TOKENS, max_frames=375)
    assert [(s.first, s.last) for s in whole] == [(0, 3)]
    # with max_frames forcing further cuts, the widest remaining pauses are used as before
    segs = longform.segments(p, TOKENS, max_frames=30)
    assert [(s.first, s.last) for s in segs] == [(0, 0), (1, 1), (2, 2), (3, 3)]
    _no_gap_frames(segs, p)
    _every_token_once(segs, p)


def test_extents_stay_out_of_gaps_at_the_ends_and_in_the_middle():
    """gap runs right up to the first word and from the last word on (margin = 5 would reach into
    them), and one covering most of a pause"""
    spans = [(1, 30, 40), (2, 44, 50), (3, 80, 90), (4, 93, 99)]
    gaps = [(0, 28), (52, 79), (100, 130)]
    p = _partial(130, spans, gaps)
    segs = longform.segments(p, TOKENS, max_frames=375, margin=5)
    assert [(s.start, s.end, s.first, s.last) for s in segs] == [(28, 52, 0, 1), (79, 100, 2, 3)]
    _no_gap_frames(segs, p)
    _every_token_once(segs, p)
    assert longform.uncovered(p) == [(0, 28), (52, 79), (100, 130)]
    # score / worst average word frames only, as for a LongAlignment
    flp = p.frame_logp
    assert segs[0].score == float(np.mean(flp[30:50], dtype=np.float64))
    assert segs[0].worst == min(float(np.mean(flp[30:40], dtype=np.float64)),
                                float(np.mean(flp[44:50], dtype=np.float64)))


@pytest.mark.parametrize("max_frames", [375, 60, 25])
def test_no_gaps_is_the_long_alignment_result(max_frames):
    rng = np.random.Generator(np.random.PCG64(3))
    t, spans = 3, []
    for i in range(40):
        n = int(rng.integers(2, 9))
        spans.append((1 + i % 10, t, t + n))
        t += n + int(rng.integers(0, 30))
    p = _partial(t + 7, spans, [])
    a = longform.LongAlignment(p.spans, p.score, p.frame_logp)
    assert longform.segments(p, TOKENS, max_frames=max_frames) == longform.segments(a, TOKENS, max_frames=max_frames)
    assert longform.uncovered(p) == []


def test_every_token_once_with_many_gaps():
    rng = np.random.Generator(np.random.PCG64(4))
    t, spans, gaps = 0, [], []
    for i in range(60):
        pause = int(rng.integers(0, 40))
        if pause >= 6 and rng.random() < 0.4:
            gaps.append((t + 2, t + pause - 1))
        t += pause
        n = int(rng.integers(2, 9))
        spans.append((1 + i % 10, t, t + n))
        t += n
    gaps.append((t + 1, t + 20))
    p = _partial(t + 20, spans, gaps)
    for max_frames in (375, 50):
        segs = longform.segments(p, TOKENS, max_frames=max_frames)
        _every_token_once(segs, p)
        _no_gap_frames(segs, p)
        for s in segs:
            assert 0 <= s.start < s.end <= len(p.ali)
            assert s.end - s.start <= max_frames or s.first == s.last
        inner = [g for g in gaps if g[0] >= spans[0][2] and g[1] <= spans[-1][1]]
        assert len(segs) >= len(inner) + 1


def test_gap_flags():
    assert longform.gap_flags(4) == [1, 0, 0, 0, 1]
    assert longform.gap_flags(4, free_start=False, gaps=(2,)) == [0, 0, 1, 0, 1]
    assert longform.gap_flags(4, False, False, "all") == [0, 1, 1, 1, 0]
    assert longform.gap_flags(0) == [1] and longform.gap_flags(0, False, False) == [0]
    assert longform.gap_flags(1, gaps="all") == [1, 1]
    for bad in ((0,), (4,), (-1,), (1.5,), "some"):
        with pytest.raises(ValueError):
            longform.gap_flags(4, gaps=bad)
    with pytest.raises(ValueError):
        longform.gap_flags(1, gaps=(1,))


class _NoDevice:
    """what align_partial reads of the model before it needs the device"""
    odim, blank, sos, eos = V, 0, V - 1, V - 1

    def engine(self):
        raise AssertionError("the argument checks come before the device")


def test_align_partial_argument_errors_need_no_device():
    e2e = _NoDevice()
    logits, lse = torch.zeros(30, V), torch.zeros(30)
    ok = dict(gap_penalty=-1.0)
    for y in ([3, V, 4], [3, -1], [3, 0, 4], [3, V - 1, 4], [1 + i % 7 for i in range(16384)]):
        with pytest.raises(ValueError):
            longform.align_partial(e2e, logits, lse, y, **ok)
    for gaps in ((0,), (3,), (7,), "every"):
        with pytest.raises(ValueError):
            longform.align_partial(e2e, logits, lse, [1, 2, 3], gaps=gaps, **ok)
    for pen in (0.1, float("nan")):
        with pytest.raises(ValueError):
            longform.align_partial(e2e, logits, lse, [1, 2, 3], gap_penalty=pen)
    with pytest.raises(ValueError):
        longform.align_partial(e2e, logits, torch.zeros(29), [1, 2, 3], **ok)
    with pytest.raises(TypeError):                               # gap_penalty has no default
        longform.align_partial(e2e, logits, lse, [1, 2, 3])
    with pytest.raises(AssertionError, match="before the device"):      # valid arguments reach the device
        longform.align_partial(e2e, logits, lse, [V - 1, 1, 2, 3, V - 1], gaps=(1, 2), **ok)

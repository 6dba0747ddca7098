"""The host side of avsr_amd.longform: the window plan of a long recording and the cutting of an
aligned recording into clips, on scripted alignments (no GPU, no model)."""
import numpy as np
import pytest

from avsr_amd import align
from avsr_amd.align import TokenSpan
from avsr_amd.longform import LongAlignment, segments, window_plan


# ------------------------------------------------------------------------------ window_plan
@pytest.mark.parametrize("window,overlap", [(375, 125), (40, 16), (40, 0), (7, 6)])
def test_window_plan_properties(window, overlap):
    for T in range(1, 1201):
        plan = window_plan(T, window, overlap)
        W = min(window, T)
        assert [p[2] for p in plan] == [0] + [p[3] for p in plan[:-1]] and plan[-1][3] == T     # keeps partition [0, T)
        for s, e, lo, hi in plan:
            assert 0 <= s and e <= T and e - s == W
            assert s <= lo < hi <= e
            # a kept frame has overlap // 2 frames of its window on each side, except at the recording's ends
            assert lo == 0 == s or lo - s >= overlap // 2
            assert hi == T == e or (e - 1) - (hi - 1) >= overlap // 2
        for (s0, e0, _, _), (s1, e1, _, _) in zip(plan, plan[1:]):
            assert s0 < s1 and e0 - s1 >= overlap
        if T <= window:
            assert plan == [(0, T, 0, T)]
        else:
            hop = window - overlap
            assert [p[0] for p in plan[:-1]] == list(range(0, T - window, hop)) and plan[-1][0] == T - window


def test_window_plan_example_and_errors():
    assert window_plan(100, 40, 16) == [(0, 40, 0, 32), (24, 64, 32, 56), (48, 88, 56, 74), (60, 100, 74, 100)]
    assert window_plan(375) == [(0, 375, 0, 375)]
    assert window_plan(376) == [(0, 375, 0, 188), (1, 376, 188, 376)]
    for bad in ((0, 375, 125), (-3, 375, 125), (100, 1, 0), (100, 40, -1), (100, 40, 40), (100, 40, 41)):
        with pytest.raises(ValueError):
            window_plan(*bad)


# ------------------------------------------------------------------------------ segments
# pieces: a word starts at a piece that begins with the space mark
TOKENS = ["<blank>", "▁a", "▁b", "c", "▁d", "▁e", "f", "g", "▁h"]


def _ali(spans, T, logp=None):
    flp = np.full(T, -1.0, dtype=np.float32) if logp is None else np.asarray(logp, dtype=np.float32)
    assert len(flp) == T
    return LongAlignment([TokenSpan(*s) for s in spans], float(flp.sum()), flp)


def test_segments_whole_when_it_fits_and_empty():
    # words: a [10, 12), bc [20, 26), d [30, 31)
    a = _ali([(1, 10, 12), (2, 20, 23), (3, 23, 26), (4, 30, 31)], 50)
    (s,) = segments(a, TOKENS, max_frames=40, margin=5)
    assert (s.start, s.end, s.first, s.last, s.tokens, s.text) == (5, 36, 0, 3, [1, 2, 3, 4], "a bc d")
    (s,) = segments(a, TOKENS, max_frames=100, margin=20)              # margins clipped by 0 and T
    assert (s.start, s.end) == (0, 50)
    assert segments(_ali([], 30), TOKENS) == []


def test_segments_split_at_the_widest_gap_and_margins():
    # words a [0, 4), bc [10, 20), d [40, 44), e [46, 50); gaps 6, 20, 2; cuts 7, 30, 45
    a = _ali([(1, 0, 4), (2, 10, 15), (3, 15, 20), (4, 40, 44), (5, 46, 50)], 60)
    segs = segments(a, TOKENS, max_frames=30, margin=5)
    assert [(s.start, s.end, s.first, s.last, s.text) for s in segs] == [(0, 25, 0, 2, "a bc"), (35, 55, 3, 4, "d e")]
    # a margin wider than half the pause stops at the cut, in both directions; and at 0 / T
    segs = segments(a, TOKENS, max_frames=35, margin=15)
    assert [(s.start, s.end) for s in segs] == [(0, 30), (30, 60)]
    # margin 0: exactly the words
    segs = segments(a, TOKENS, max_frames=30, margin=0)
    assert [(s.start, s.end) for s in segs] == [(0, 20), (40, 50)]


def test_segments_tie_goes_to_the_lower_index():
    # words at [0, 10), [20, 30), [40, 50): both gaps 10
    a = _ali([(1, 0, 10), (4, 20, 30), (8, 40, 50)], 50)
    segs = segments(a, TOKENS, max_frames=35, margin=0)
    assert [(s.first, s.last, s.start, s.end) for s in segs] == [(0, 0, 0, 10), (1, 2, 20, 50)]


def test_segments_recursion_to_three_levels_and_an_overlong_word():
    # words (start, end): a (0, 5), d (25, 30), h (60, 65), a (75, 80), d (82, 88), e.f.g (100, 160), h (161, 170)
    # gaps 20, 30, 10, 2, 12, 1: level 1 splits at the 30, level 2 at the 12 (and the 20 on the left),
    # level 3 at the 10 of (h, a, d); the 60-frame word stays whole, longer than max_frames
    sp = [(1, 0, 5), (4, 25, 30), (8, 60, 65), (1, 75, 80), (4, 82, 88), (5, 100, 120), (6, 120, 140), (7, 140, 160),
          (8, 161, 170)]
    a = _ali(sp, 170)
    segs = segments(a, TOKENS, max_frames=25, margin=2)
    assert [(s.first, s.last) for s in segs] == [(0, 0), (1, 1), (2, 2), (3, 4), (5, 7), (8, 8)]
    assert [s.text for s in segs] == ["a", "d", "h", "a d", "efg", "h"]
    assert [(s.start, s.end) for s in segs] == [(0, 7), (23, 32), (58, 67), (73, 90), (98, 160), (160, 170)]
    assert segs[4].end - segs[4].start > 25 and all(s.end - s.start <= 25 for i, s in enumerate(segs) if i != 4)
    # every token exactly once, in order, and the words are those of align.word_groups
    assert [t for s in segs for t in s.tokens] == [t for t, _, _ in sp]
    words = [w for w, _ in align.word_groups([t for t, _, _ in sp], TOKENS)]
    assert " ".join(s.text for s in segs).split() == words
    for s in segs:
        assert s.tokens == [t for t, _, _ in sp[s.first:s.last + 1]]


def test_segments_score_and_worst():
    # words a [2, 4), bc [6, 10); frame log-probs are multiples of 1/4: the means are exact
    flp = [-9, -9, -1.0, -2.0, -8, -8, -0.5, -0.5, -3.0, -4.0, -9, -9]
    a = _ali([(1, 2, 4), (2, 6, 8), (3, 8, 10)], 12, flp)
    (s,) = segments(a, TOKENS, max_frames=100, margin=1)
    assert (s.start, s.end) == (1, 11)
    assert s.score == (-1.0 - 2.0 - 8 - 8 - 0.5 - 0.5 - 3.0 - 4.0) / 8          # [start_a, end_b): the pause counts
    assert s.worst == min((-1.0 - 2.0) / 2, (-0.5 - 0.5 - 3.0 - 4.0) / 4) == -2.0
    s0, s1 = segments(a, TOKENS, max_frames=5, margin=0)
    assert (s0.score, s0.worst, s1.score, s1.worst) == (-1.5, -1.5, -2.0, -2.0)

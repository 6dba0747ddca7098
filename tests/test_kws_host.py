"""Host side of keyword spotting, no GPU: the numpy reference of avsr_ctc_kws (tests/kws_ref.py)
against the brute force over all spans, its tie and infeasibility rules, and the pure host code of
avsr_amd.kws (select_occurrences, check_keywords, hit_times)."""
import math

import numpy as np
import pytest

from avsr_amd import kws
from tests import kws_ref as R


def _logp(rng, T, V):
    x = rng.standard_normal((T, V)) * 3
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def _plant(T, V, frames, hot=10.0):
    """log-probs whose argmax is frames[t] (a token id per frame)"""
    x = np.zeros((T, V))
    x[np.arange(T), frames] = hot
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


@pytest.mark.parametrize("filler", [True, False])
def test_reference_equals_brute_force(filler):
    """fp64: the free-start / free-end DP is the maximum over all spans of the pinned Viterbi;
    labels from 3 ids, so adjacent repeats (no skip, a blank needed) occur"""
    rng = np.random.Generator(np.random.PCG64(11))
    V, seen_rep, seen_inf = 12, 0, 0
    for _ in range(120):
        T, L = int(rng.integers(1, 14)), int(rng.integers(1, 5))
        y = rng.integers(1, 4, size=L).tolist()
        lp = _logp(rng, T, V)
        top = lp.argmax(-1) if filler else None
        got = R.spot(lp, y, T, top, dtype=np.float64)
        want = R.brute_force(lp, y, T, top)
        seen_rep += any(a == b for a, b in zip(y, y[1:]))
        if want == -np.inf:
            seen_inf += 1
            assert got[0] == -np.inf and got[1] == got[2] == -1
            continue
        assert abs(got[0] - want) <= 1e-9, (y, T, got[0], want)
        s, e = got[1], got[2]
        assert 0 <= s < e <= T
        # the span it reports carries the score it reports
        ext = np.zeros(2 * L - 1, dtype=np.int64)
        ext[0::2] = y
        skip = np.zeros(len(ext), dtype=bool)
        skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
        f = lp[np.arange(T), top] if filler else np.zeros(T)
        assert abs(R.pinned((lp[:, ext] - f[:, None])[s:e], ext, skip) - want) <= 1e-9
    assert seen_rep > 20 and seen_inf > 5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_keyword(dtype):
    """(5, 5, 9) said over frames 6..13 of 20 (5 5 5 _ 5 5 9 9): the span is [6, 14), and against
    the filler its score is exactly 0"""
    frames = [0] * 6 + [5, 5, 5, 0, 5, 5, 9, 9] + [0] * 6
    lp = _plant(20, 12, frames)
    score, start, end, trace, tstart = R.spot(lp, (5, 5, 9), 20, lp.argmax(-1), dtype=dtype)
    assert (score, start, end) == (0.0, 6, 14)
    assert trace[13] == 0.0 and tstart[13] == 6 and trace[12] == 0.0 and (trace[:12] < 0).all()


def test_too_few_frames():
    """13 equal labels need 25 frames"""
    lp = _logp(np.random.Generator(np.random.PCG64(1)), 25, 12).astype(np.float32)
    score, start, end, trace, tstart = R.spot(lp, [3] * 13, 23, lp.argmax(-1))
    assert score == -np.inf and start == -1 and end == -1
    assert (trace == -np.inf).all() and (tstart == -1).all()
    assert R.spot(lp, [3] * 13, 25, lp.argmax(-1))[0] > -np.inf
    for bad in ([], [0], [12], [-1], [3, 0, 4]):                 # empty, blank, outside [0, V)
        assert R.spot(lp, bad, 25, lp.argmax(-1))[0] == -np.inf


@pytest.mark.parametrize("y", [(3,), (3, 4), (3, 3), (5, 1, 5, 5)])
def test_all_ties(y):
    """constant logits: every path ties at 0, and the rules (strict comparisons in the order stay,
    s-1, s-2, enter; the last best end) give the whole utterance"""
    T = 11
    lp = np.full((T, 12), -math.log(12), dtype=np.float32)
    score, start, end, _, _ = R.spot(lp, y, T, np.zeros(T, dtype=np.int64))
    assert (score, start, end) == (0.0, 0, T)


def _traces(frames, y, T, V=12):
    lp = _plant(T, V, frames)
    return R.spot(lp, y, T, lp.argmax(-1))


def test_select_occurrences():
    # (5, 9) said twice: frames 3..6 (5 5 9 9) and 12..14 (5 _ 9)... the blank between is not needed
    frames = [0] * 3 + [5, 5, 9, 9] + [0] * 5 + [5, 9, 9] + [0] * 5
    T = len(frames)
    score, start, end, trace, tstart = _traces(frames, (5, 9), T)
    occ = kws.select_occurrences(trace, tstart, threshold=-1.0, keyword=4)
    # two occurrences, in start order; the candidates ending at 6 and 7 (and 14, 15) of one
    # occurrence overlap and collapse into the later end
    assert [(h.start, h.end) for h in occ] == [(3, 7), (12, 15)]
    assert all(h.keyword == 4 and h.score == 0.0 and h.avg == 0.0 for h in occ)
    # the first accepted candidate is the kernel's best (score descending, later end first)
    assert (start, end) == (12, 15) and score == 0.0
    best = max(occ, key=lambda h: (h.score, h.end))
    assert (best.start, best.end, best.score) == (start, end, float(score))
    # no threshold: every finite candidate competes, so the gaps fill with poor occurrences; the
    # good ones are still there and nothing overlaps
    every = kws.select_occurrences(trace, tstart)
    assert {(3, 7), (12, 15)} <= {(h.start, h.end) for h in every}
    assert all(a.end <= b.start for a, b in zip(every, every[1:]))
    # the threshold applies to avg = score / frames, not to score
    tr = np.array([-np.inf, -4.0, -4.0, -np.inf, -np.inf, -np.inf, -np.inf, -6.0], dtype=np.float32)
    ts = np.array([-1, 0, 2, -1, -1, -1, -1, 3], dtype=np.int32)
    # candidates: [0, 2) avg -2; [2, 3) avg -4; [3, 8) avg -1.2 (the worst score, the best avg)
    got = kws.select_occurrences(tr, ts, threshold=-2.0)
    assert [(h.start, h.end, h.score, h.avg) for h in got] == [(0, 2, -4.0, -2.0), (3, 8, -6.0, -1.2)]
    assert [(h.start, h.end) for h in kws.select_occurrences(tr, ts, threshold=-1.5)] == [(3, 8)]
    # ties in score: the later end wins, and the overlapped one is dropped
    got = kws.select_occurrences(np.array([-1.0, -1.0], np.float32), np.array([0, 0], np.int32))
    assert [(h.start, h.end) for h in got] == [(0, 2)]
    assert kws.select_occurrences(np.full(5, -np.inf, np.float32), np.full(5, -1, np.int32)) == []


def test_check_keywords():
    V, blank, eos = 50, 0, 49
    assert kws.check_keywords([(1, 2), np.array([3])], V, blank, eos) == [[1, 2], [3]]
    assert kws.check_keywords([[7] * 32], V, blank, eos) == [[7] * 32]
    for bad in ([], [[]], [[1], []], [[0]], [[1, 49]], [[-1]], [[50]], [[7] * 33]):
        with pytest.raises(ValueError):
            kws.check_keywords(bad, V, blank, eos)


def test_hit_times():
    h = kws.KeywordHit(0, 6, 14, -1.0, -0.125)
    assert kws.hit_times(h) == (0.24, 0.56) and kws.hit_times(h, frame_rate=50.0) == (0.12, 0.28)

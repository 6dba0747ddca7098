"""tests/align_gaps_ref.py, the host reference of the avsr_ctc_align_gaps tests: without flags, or
with gap_penalty = -inf, it is tests/align_long_ref.viterbi bit for bit; on the two planted cases
(a transcript inside a longer recording; two halves with untranscribed speech between them) it
finds the planted frames; its score is the gap-aware sequential path sum; gap frames lie only
where a flag allows them."""
import numpy as np
import pytest
import torch

from tests import align_gaps_ref as G
from tests import align_long_ref as R

NINF = -float("inf")


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("launch", R.launches(), ids=lambda l: l[0])
def test_no_flags_or_minus_inf_is_the_plain_viterbi(launch, dtype):
    _, cases, T, kw = launch
    x, lse = R.inputs(cases, T, 64, 72, dtype, **kw)
    x, lse = x.float().numpy(), lse.numpy()
    ys, Ts = [y for _, y in cases], [Tb for Tb, _ in cases]
    fil = G.filler_of(x, lse, 64)
    want = R.align_batch(x, lse, ys, Ts, T)
    for gaps, pen in (([np.zeros(len(y) + 1, np.uint8) for y in ys], -0.5),
                      ([np.ones(len(y) + 1, np.uint8) for y in ys], NINF)):
        got = G.align_batch(x, lse, fil, ys, gaps, pen, Ts, T)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
        assert got[1].dtype == np.float32 and np.array_equal(_bits(got[1]), _bits(want[1]))


def _planted(case, flags=None, pen=-1.0):
    x, lse, fil, truth = G.planted(case["segments"], case["T"], case["seed"])
    y = case["y"]
    g = G.flags_at(len(y), case["flags"] if flags is None else flags)
    ali, score, feas = G.viterbi(x, lse, fil, y, g, pen, case["T"])
    assert feas == 1
    return x, lse, fil, truth, g, ali, score


def _only_in_flagged_stretches(ali, y, g):
    """a GAP frame lies between the tokens (or ends) that a set flag separates: the number of
    label starts before a GAP frame is a flagged position"""
    from avsr_amd import align
    lab = np.where(ali == G.GAP, 0, ali)
    spans = align.token_spans(lab, 0)
    assert [sp.token for sp in spans] == list(y)
    pos = np.zeros(len(ali), dtype=np.int64)
    for sp in spans:
        pos[sp.start:] += 1
    assert all(g[pos[t]] for t in np.nonzero(ali == G.GAP)[0])


def test_free_ends_find_the_planted_transcript():
    x, lse, fil, truth, g, ali, score = _planted(G.FREE_ENDS)
    y, T = G.FREE_ENDS["y"], G.FREE_ENDS["T"]
    lab = np.nonzero(ali > 0)[0]
    assert lab[0] == 40 and lab[-1] < 80
    assert (ali == G.GAP).sum() == 80
    plain, pscore, _ = R.viterbi(x, lse, y, T)
    assert score > pscore and np.nonzero(plain > 0)[0][0] < 40          # fixed ends smear the first word
    assert round(float(score), 1) == -86.0 and round(float(pscore), 1) == -645.7
    assert _bits(score) == _bits(G.path_sum(x, lse, fil, -1.0, ali))
    _only_in_flagged_stretches(ali, y, g)
    assert G.gap_runs(ali)[0][0] == 0 and G.gap_runs(ali)[-1][1] == T


@pytest.mark.parametrize("flags", [None, range(9)], ids=["0-4-8", "all"])
def test_mid_gap_keeps_every_token_on_its_planted_frames(flags):
    x, lse, fil, truth, g, ali, score = _planted(G.MID_GAP, flags)
    y = G.MID_GAP["y"]
    for i, k in enumerate(y):
        assert np.nonzero(ali == k)[0].tolist() == list(range(*truth[i])), (i, k)
    assert _bits(score) == _bits(G.path_sum(x, lse, fil, -1.0, ali))
    _only_in_flagged_stretches(ali, y, g)
    assert any(lo >= truth[3][1] and hi <= truth[4][0] for lo, hi in G.gap_runs(ali))


def test_score_is_the_gap_aware_path_sum_at_size():
    T, L = 1600, 700
    y = R.random_labels(L, 31, repeats=(100, 101, 650))
    x, lse = R.inputs([(T, y)], T, 64, 72, torch.float32, seed=32)
    x, lse = x.numpy(), lse.numpy()
    fil = G.filler_of(x, lse, 64)
    g = G.random_flags(L, 33)
    ali, score, feas = G.viterbi(x, lse, fil, y, g, -0.5, T)
    assert feas == 1 and (ali == G.GAP).any()
    assert _bits(score) == _bits(G.path_sum(x, lse, fil, -0.5, ali))
    _only_in_flagged_stretches(ali, y, g)
    e = G.frame_terms(x, lse, fil, -0.5, ali)
    assert (e[ali == G.GAP] > (x[:, 0] - lse)[ali == G.GAP]).all()      # strictly above the blank


def test_strict_compare_prefers_blank_on_a_tie():
    """ef == eb: the blank, no GAP"""
    x = np.zeros((4, 8), np.float32)
    x[:, 0] = 2.0
    lse = np.zeros(4, np.float32)
    fil = np.full(4, 2.0, np.float32)
    ali, score, feas = G.viterbi(x, lse, fil, (), [1], 0.0, 4)
    assert feas == 1 and ali.tolist() == [0, 0, 0, 0] and score == 8.0
    ali, _, _ = G.viterbi(x, lse, fil + np.float32(0.5), (), [1], 0.0, 4)
    assert ali.tolist() == [G.GAP] * 4

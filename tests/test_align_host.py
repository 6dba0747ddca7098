"""Host side of CTC forced alignment (no GPU): the float32 numpy Viterbi the GPU tests use as
their reference (tests/align_ref.py) reproduces every alignment the reference's
CTC.forced_align_batch returned (tests/golden/avsr_align.npz, make_golden_align.py), and the
span / word-time helpers of avsr_amd.align."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from avsr_amd.align import TokenSpan, strip_sos_eos, token_spans, word_times
from tests.align_ref import align_batch, viterbi
from tests.oracle_util import golden_state, load_golden

GOLDEN_ALIGN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avsr_align.npz")


@pytest.fixture(scope="module")
def ga():
    return dict(np.load(GOLDEN_ALIGN, allow_pickle=False))


@pytest.fixture(scope="module")
def ctc_lo():
    st = golden_state(load_golden())
    return torch.from_numpy(st["avsr.ctc.ctc_lo.weight"]), torch.from_numpy(st["avsr.ctc.ctc_lo.bias"])


@pytest.mark.parametrize("k", [1, 2])
def test_helper_reproduces_reference_alignments(ga, ctc_lo, k):
    hs, ys_pad, ilens, want = ga[f"hs{k}"], ga[f"ys_pad{k}"], ga[f"ilens{k}"], ga[f"ali{k}"]
    B, T, _ = hs.shape
    lp = torch.log_softmax(F.linear(torch.from_numpy(hs), *ctc_lo), -1).numpy()
    labels = [r[r != -1].tolist() for r in ys_pad]
    ali, score, feas = align_batch(lp.reshape(B * T, -1), np.zeros(B * T, np.float32), labels, ilens, T)
    assert feas.tolist() == [1] * B
    assert np.array_equal(ali, want.astype(np.int32))
    assert ali.dtype == np.int32 and score.dtype == np.float32
    # the stored fp64 path scores: fp32 sums of T <= 25 log-probs of magnitude ~10
    assert np.allclose(score, ga[f"score{k}"], rtol=1e-5, atol=0)


def test_helper_edge_cases():
    rng = np.random.Generator(np.random.PCG64(0))
    x = rng.standard_normal((9, 8)).astype(np.float32)
    z = np.zeros(9, np.float32)
    # infeasible: T < L + adjacent repeats; T = 0
    assert viterbi(x, z, (3, 3, 5), 3)[2] == 0 and viterbi(x, z, (3,), 0)[2] == 0
    a, _, f = viterbi(x, z, (3, 3, 5), 4)
    assert f == 1 and a.tolist() == [3, 0, 3, 5]
    # L = 0: all blanks, score = sum of the blank column
    a, s, f = viterbi(x, z, (), 5)
    assert f == 1 and a.tolist() == [0] * 5
    acc = np.float32(x[0, 0])
    for t in range(1, 5):
        acc = np.float32(acc + x[t, 0])
    assert s == acc
    # all ties: the final state is the first maximum of (S-2, S-1), the last label; the first
    # maximum in (s, s-1, s-2) keeps the backtrack in a state for as long as it was reachable,
    # so the path runs to its final state as early as it can and stays there
    a, _, f = viterbi(np.zeros((9, 8), np.float32), z, (3, 3, 5), 9)
    assert f == 1 and a.tolist() == [3, 0, 3, 5, 5, 5, 5, 5, 5]


def test_token_spans():
    S = TokenSpan
    # a repeat through a blank: two tokens
    assert token_spans([7, 7, 0, 7, 3]) == [S(7, 0, 2), S(7, 3, 4), S(3, 4, 5)]
    # adjacent distinct tokens without a blank
    assert token_spans([1, 2, 2, 3]) == [S(1, 0, 1), S(2, 1, 3), S(3, 3, 4)]
    # leading and trailing blanks
    assert token_spans([0, 0, 5, 5, 0, 9, 0, 0]) == [S(5, 2, 4), S(9, 5, 6)]
    # all blank, empty
    assert token_spans([0, 0, 0]) == [] and token_spans([]) == []
    # another blank id; numpy input
    assert token_spans(np.array([4, 1, 1, 4, 0]), blank=4) == [S(1, 1, 3), S(0, 4, 5)]
    assert all(isinstance(v, int) for sp in token_spans(np.array([0, 2, 2])) for v in sp)


def test_strip_sos_eos():
    assert strip_sos_eos([9, 1, 2, 9], 9, 9) == [1, 2]
    assert strip_sos_eos([1, 2], 9, 9) == [1, 2]
    assert strip_sos_eos(torch.tensor([9, 1]), 9, 9) == [1]
    assert strip_sos_eos([9, 9], 9, 9) == [] and strip_sos_eos([], 9, 9) == []


def test_word_times():
    tokens = ["<blank>", "▁he", "llo", "▁wor", "ld", "▁a", "x"]
    spans = [TokenSpan(1, 2, 4), TokenSpan(2, 4, 5), TokenSpan(3, 10, 12), TokenSpan(4, 12, 13), TokenSpan(5, 20, 25)]
    assert word_times(spans, tokens) == [("hello", 0.08, 0.2), ("world", 0.4, 0.52), ("a", 0.8, 1.0)]
    assert word_times(spans[:2], tokens, frame_rate=50.0) == [("hello", 0.04, 0.1)]
    # a first piece without the word marker still opens a word
    assert word_times([TokenSpan(6, 0, 5), TokenSpan(2, 5, 10)], tokens, frame_rate=5.0) == [("xllo", 0.0, 2.0)]
    assert word_times([], tokens) == []
    assert word_times([TokenSpan(1, 0, 5)], ["<blank>", "_he"], frame_rate=5.0, space="_") == [("he", 0.0, 1.0)]

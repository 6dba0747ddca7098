"""tests/align_long_ref.py, the host reference of the avsr_ctc_align_long tests, against
tests/align_ref.viterbi (the reference of the avsr_ctc_align tests): equal on the launches of
tests/test_gpu_align.py and past the old kernel's bound, and the path-sum identity that the GPU
test relies on at L = 16383, where no host Viterbi is run."""
import numpy as np
import pytest
import torch

from tests import align_long_ref as R
from tests import align_ref


def _equal(x, lse, cases, T, blank=0):
    x, lse = x.float().numpy(), lse.numpy()
    ys, Ts = [y for _, y in cases], [Tb for Tb, _ in cases]
    got = R.align_batch(x, lse, ys, Ts, T, blank)
    want = align_ref.align_batch(x, lse, ys, Ts, T, blank)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
    assert got[1].dtype == want[1].dtype == np.float32
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("launch", R.launches(), ids=lambda l: l[0])
def test_equals_align_ref_on_the_old_launches(launch, dtype):
    _, cases, T, kw = launch
    x, lse = R.inputs(cases, T, 64, 72, dtype, **kw)
    _equal(x, lse, cases, T)


def test_equals_align_ref_past_the_old_bound_and_with_another_blank():
    y = R.random_labels(513, 7, repeats=(20, 21, 300))
    cases = [(1300, y)]
    x, lse = R.inputs(cases, 1300, 64, 72, torch.float32, seed=8)
    _, _, feas = _equal(x, lse, cases, 1300)
    assert feas.tolist() == [1]
    cases = [(12, (7, 7, 0, 3)), (12, (1, 2))]
    x, lse = R.inputs(cases, 12, 64, 72, torch.float32, seed=4)
    _equal(x, lse, cases, 12, blank=5)


def test_score_is_the_sequential_path_sum():
    """score == the float32 sum, in frame order, of x[t][ali[t]] - lse[t], bit for bit, with the
    Viterbi of align_ref: the identity that stands in for the host Viterbi at L = 16383"""
    T, L = 3200, 1500
    y = R.random_labels(L, 9, repeats=(100, 101, 700, 1400))
    x, lse = R.inputs([(T, y)], T, 64, 72, torch.float32, seed=10)
    x, lse = x.numpy(), lse.numpy()
    ali, score, feas = align_ref.viterbi(x, lse, y, T)
    assert feas == 1 and score.dtype == np.float32
    s = R.path_sum(x, lse, ali)
    assert s.dtype == np.float32 and s.view(np.int32) == score.view(np.int32), (s, score)
    ali2, score2, _ = R.viterbi(x, lse, y, T)
    assert np.array_equal(ali, ali2) and score2.view(np.int32) == score.view(np.int32)

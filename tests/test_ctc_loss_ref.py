"""tests/ctc_loss_ref.py against torch's CPU CTC in fp64, on every utterance of the case tables
that tests/test_gpu_loss_edges.py runs on the device. No GPU."""
import pytest
import torch

from tests import ctc_loss_ref as R


def _close(a, b, rel):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() <= rel * b.abs().max().item()


@pytest.mark.parametrize("name,regime", R.all_ctc_cases())
def test_ctc_ref_matches_torch_fp64(name, regime):
    c = R.CTC_CASES[name]
    T, V = c["T"], c["V"]
    x = R.case_logits(name, regime)
    assert torch.isnan(x[:, :, V:]).all() and torch.isfinite(x[:, :, :V]).all()
    for b, (labels, in_len) in enumerate(c["utts"]):
        xb = x[b, :, :V].double()
        nll, alpha, gamma, grad = R.ctc_ref(xb, labels, in_len)
        Tb, S = max(0, min(in_len, T)), 2 * len(labels) + 1
        assert alpha.shape == (Tb, S) and gamma.shape == (T, S) and grad.shape == (T, V)
        ok = R.feasible(labels, in_len, T)
        assert (nll.item() > 0) == ok
        if not ok:
            assert not alpha.any() and not gamma.any() and not grad.any()
        else:
            assert (gamma[:Tb].sum(1) - 1).abs().max().item() < 1e-9
            assert not gamma[Tb:].any() and not grad[Tb:].any()
        if in_len < 1:
            continue
        tnll, tgrad = R.torch_ctc(xb, labels, in_len, torch.float64)
        assert _close(nll, tnll, 1e-9), (b, nll.item(), tnll.item())
        assert _close(grad, tgrad, 1e-9), (b, (grad - tgrad).abs().max().item())


def test_ctc_ref_fp32_is_the_same_recursion():
    """dtype=float32 runs in fp32 and lands within fp32 rounding of fp64"""
    labels, in_len = R.CTC_CASES["chunk-edges"]["utts"][1]
    xb = R.case_logits("chunk-edges", "random")[1, :, :50]
    out64 = R.ctc_ref(xb, labels, in_len)
    out32 = R.ctc_ref(xb, labels, in_len, dtype=torch.float32)
    assert all(o.dtype == torch.float32 for o in out32)
    assert abs(out32[0].item() - out64[0].item()) < 1e-5 * out64[0].item()
    assert 0 < (out32[2].double() - out64[2]).abs().max().item() < 1e-3


def test_planted_alignment():
    assert R.planted_alignment([2, 2, 3], 6) == [2, 0, 2, 3, 0, 0]
    assert R.planted_alignment([2, 2, 3], 3) == [2, 0, 2]
    assert R.planted_alignment([], 2) == [0, 0]

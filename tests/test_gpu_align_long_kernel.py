"""avsr_ctc_align_long, the CTC forced alignment of whole recordings, against the float32 host
Viterbi of tests/align_long_ref.py (same arithmetic, same order: exact equality, no tolerance)
and against avsr_ctc_align where both kernels apply. Logits are 1e30 outside the valid columns
and frames; outputs and workspace start as garbage."""
import numpy as np
import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import align, ops
from tests import align_long_ref as R

pytestmark = pytest.mark.gpu

V, LDX = 64, 72


def _labels(cases):
    B = len(cases)
    Lmax = max(1, max(len(y) for _, y in cases))
    lab = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, (_, y) in enumerate(cases):
        lab[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
    return lab, torch.tensor([len(y) for _, y in cases], dtype=torch.int32), \
        torch.tensor([Tb for Tb, _ in cases], dtype=torch.int32)


def _launch(dev, x, lse, cases, T, V=V, blank=0, old=False, ws_shift=0):
    """ops.ctc_align_long (old: ops.ctc_align) with outputs and workspace pre-filled with garbage:
    every element must be written, none may be read"""
    B = len(cases)
    lab, llen, ilen = _labels(cases)
    ali = torch.full((B, T), 7777, dtype=torch.int32, device=dev)
    score = torch.full((B,), 7777.0, device=dev)
    feas = torch.full((B,), 7777, dtype=torch.int32, device=dev)
    nbytes = (ops.ctc_align_ws if old else ops.ctc_align_long_ws)(B, T, lab.shape[1])
    ws = torch.full((max(16, nbytes) + 16,), 255, dtype=torch.uint8, device=dev)[ws_shift:ws_shift + max(16, nbytes)]
    (ops.ctc_align if old else ops.ctc_align_long)(x.to(dev), B, T, V, lab.to(dev), llen.to(dev), ilen.to(dev),
                                                  lse.to(dev), blank=blank, ali=ali, score=score, feasible=feas, ws=ws)
    return ali.cpu(), score.cpu(), feas.cpu()


def _reference(x, lse, cases, T, blank=0):
    ali, score, feas = R.align_batch(x.float().numpy(), lse.numpy(), [y for _, y in cases], [Tb for Tb, _ in cases],
                                     T, blank)
    return torch.from_numpy(ali), torch.from_numpy(score), torch.from_numpy(feas)


def _same(got, want):
    """ali equal, score bit-equal, feasible equal"""
    assert torch.equal(got[2], want[2]), (got[2], want[2])
    assert torch.equal(got[0], want[0]), (got[0] != want[0]).nonzero()[:8]
    assert got[1].dtype == want[1].dtype == torch.float32
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (got[1], want[1])


def _check(dev, cases, T, dtype=torch.float32, V=V, ldx=LDX, blank=0, **kw):
    x, lse = R.inputs(cases, T, V, ldx, dtype, **kw)
    got = _launch(dev, x, lse, cases, T, V=V, blank=blank)
    _same(got, _reference(x, lse, cases, T, blank))
    return got


def _is_alignment_of(ali, cases):
    for b, (Tb, y) in enumerate(cases):
        assert [sp.token for sp in align.token_spans(ali[b, :Tb])] == list(y)
        assert (ali[b, max(Tb, 0):] == -1).all()


# ---------------------------------------------------------------- where both kernels apply
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("launch", R.launches(), ids=lambda l: l[0])
def test_same_as_the_old_kernel(dev, launch, dtype):
    """the four launches of tests/test_gpu_align.py (ragged; infeasible rows between feasible
    ones; S = 261 and S = 1023; all ties): equal to the host reference and to ops.ctc_align"""
    _, cases, T, kw = launch
    x, lse = R.inputs(cases, T, V, LDX, dtype, **kw)
    got = _launch(dev, x, lse, cases, T)
    _same(got, _reference(x, lse, cases, T))
    _same(got, _launch(dev, x, lse, cases, T, old=True))


@pytest.mark.parametrize("L_", [512, 513])
def test_past_the_old_bound(dev, L_):
    """L = 512 is the old kernel's shape error; here it and L = 513 are alignments"""
    cases = [(700, R.random_labels(L_, 11, repeats=(5, 6, 400)))]
    ali, _, feas = _check(dev, cases, 700, seed=12)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)


# ---------------------------------------------------------------- layout edges
@pytest.mark.parametrize("L_", [2047, 2048, 4095, 4096, 8191, 8192])
def test_layout_edges(dev, L_):
    """a thread holds P = 4 / 8 / 16 / 32 states and stores a byte / ushort / dword / two dwords of
    pointers per frame, chosen from S = 2 Lmax + 1 against 4096 / 8192 / 16384: L = 2047 | 2048,
    4095 | 4096 and 8191 | 8192 are the two sides of each edge (S = 4095 fills the 1024 threads of
    P = 4 but for one state, S = 4097 leaves thread 512 of P = 8 with one). T = L + adjacent
    repeats + 50, with one more repeat where that makes T odd: no multiple of the prefetch depth
    (4; 2 at P = 32) or of the 256-frame backtrack chunk."""
    y = list(R.random_labels(L_, L_, repeats=(3, 4, L_ // 2, L_ - 2)))
    i = 10
    while (L_ + R.n_repeats(y) + 50) % 2 == 0:
        y[i + 1] = y[i]
        i += 3
    y = tuple(y)
    T = L_ + R.n_repeats(y) + 50
    assert T % 2 == 1
    cases = [(T, y)]
    ali, _, feas = _check(dev, cases, T, seed=L_)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)


def test_one_frame_and_prefetch_tails(dev):
    """T = 1 (no pointer row at all), and T = 2, 3, 5, 6, 7 around the prefetch depth of 4"""
    for T, y in ((1, (4,)), (1, ()), (2, (4,)), (3, (4, 9)), (5, (4, 4, 9)), (6, (1, 2, 3)), (7, (1, 1, 1, 1))):
        ali, _, feas = _check(dev, [(T, y)], T, seed=T)
        assert feas.tolist() == [1]
        _is_alignment_of(ali, [(T, y)])


def test_middle_size_with_slack(dev):
    y = R.random_labels(1500, 13, repeats=(100, 101, 700, 1400))         # one triple
    cases = [(3200, y)]
    ali, _, feas = _check(dev, cases, 3200, seed=14)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)


# ---------------------------------------------------------------- the bound
def test_the_bound(dev):
    """L = 16383 (S = 32767, the widest layout), T = 16500: a feasible alignment of y whose score is
    the sequential float32 sum along its own path (tests/test_align_long_ref.py: that is what a
    Viterbi score is, bit for bit); its optimality is what the smaller cases establish. L = 16384
    is the shape error."""
    T, Tp = 16500, 16520
    y = R.random_labels(16383, 15, distinct=True)
    cases = [(T, y)]
    x, lse = R.inputs(cases, Tp, V, LDX, torch.float32, seed=16)
    ali, score, feas = _launch(dev, x, lse, cases, Tp)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)
    want = R.path_sum(x.numpy(), lse.numpy(), ali[0, :T].numpy())
    assert score.numpy()[0].view(np.int32) == want.view(np.int32), (score, want)
    bad = [(T, y + (5,))]
    with pytest.raises(L.AvsrLibError, match="1001"):            # AVSR_E_SHAPE
        _launch(dev, x, lse, bad, Tp)


# ---------------------------------------------------------------- ties, unreachable states
def test_ties_at_size(dev):
    """lse = 0 and logits that are multiples of 0.5: path sums are exact, so thousands of paths
    tie exactly and the first-maximum rule decides"""
    y = R.random_labels(1200, 17, repeats=(10, 600))
    cases = [(1500, y)]
    x, _ = R.inputs(cases, 1500, V, LDX, torch.float32, seed=18, quant=0.5)
    lse = torch.zeros(1500)
    got = _launch(dev, x, lse, cases, 1500)
    _same(got, _reference(x, lse, cases, 1500))
    assert got[2].tolist() == [1]


def test_unreachable_states(dev):
    """-inf logits in one label's column over a stretch of frames: no NaN, equal to the reference;
    over every frame: no path, feasible = 0, ali = -1, score = 0"""
    y = (5, 17, 30, 42, 40, 9, 17, 3)
    cases = [(60, y)]
    x, lse = R.inputs(cases, 60, V, LDX, torch.float32, seed=19)
    x[10:35, 30] = -float("inf")
    got = _launch(dev, x, lse, cases, 60)
    _same(got, _reference(x, lse, cases, 60))
    assert got[2].tolist() == [1] and torch.isfinite(got[1]).all()
    _is_alignment_of(got[0], cases)
    x[:, 30] = -float("inf")
    ali, score, feas = _launch(dev, x, lse, cases, 60)
    assert feas.tolist() == [0] and ali[0].tolist() == [-1] * 60 and score[0].item() == 0.0


# ---------------------------------------------------------------- batch, other parameters
def test_batch_rows_equal_their_own_launch(dev):
    """B = 3, T padded to 700: different in_len and label_len, one infeasible row (fewer frames
    than labels), one with L = 0; Lmax = 600 for all of them"""
    T = 700
    cases = [(650, R.random_labels(600, 20, repeats=(7,))), (90, R.random_labels(100, 21)), (333, ())]
    x, lse = R.inputs(cases, T, V, LDX, torch.float32, seed=22)
    got = _launch(dev, x, lse, cases, T)
    _same(got, _reference(x, lse, cases, T))
    assert got[2].tolist() == [1, 0, 1]
    assert got[0][1].tolist() == [-1] * T and got[1][1].item() == 0.0
    assert got[0][2].tolist() == [0] * 333 + [-1] * (T - 333)
    for b in range(3):
        alone = _launch(dev, x[b * T:(b + 1) * T], lse[b * T:(b + 1) * T], cases[b:b + 1], T)
        _same(alone, tuple(o[b:b + 1] for o in got))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_vocabulary(dev, dtype):
    """the model's V = 5049 / ldx = 5056 with ids up to 5047 at L = 600"""
    y = list(R.random_labels(600, 23, hi=5048))
    y[0], y[300], y[599] = 5047, 5047, 5047
    cases = [(700, tuple(y))]
    ali, _, feas = _check(dev, cases, 700, dtype=dtype, V=5049, ldx=5056, seed=24)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)


def test_other_blank_and_bad_label(dev):
    """blank is a parameter; a label of 64 (= V) or of -1 makes only its own row infeasible"""
    cases = [(12, (7, 7, 0, 3)), (12, (1, 2))]
    _check(dev, cases, 12, blank=5, seed=4)
    cases = [(12, (7, 64, 3)), (12, (1, 2)), (12, (-1, 2))]
    x, lse = R.inputs(cases, 12, V, LDX, torch.float32, seed=4)
    ali, score, feas = _launch(dev, x, lse, cases, 12)
    assert feas.tolist() == [0, 1, 0]
    for b in (0, 2):
        assert ali[b].tolist() == [-1] * 12 and score[b].item() == 0.0
    _same((ali[1:2], score[1:2], feas[1:2]), _reference(x[12:24], lse[12:24], cases[1:2], 12))


def test_workspace_alignment(dev):
    """the workspace is 16-byte aligned: one dword (the unit of the old kernel's workspace) or one
    byte off is AVSR_E_ALIGN"""
    cases = [(25, R.Y6)]
    x, lse = R.inputs(cases, 25, V, LDX, torch.float32)
    _launch(dev, x, lse, cases, 25, ws_shift=0)
    for shift in (1, 4, 8):
        with pytest.raises(L.AvsrLibError, match="1002"):        # AVSR_E_ALIGN
            _launch(dev, x, lse, cases, 25, ws_shift=shift)
    assert ops.ctc_align_long_ws(1, 30000, 6000) == 30000 * 3008 and ops.ctc_align_long_ws(2, 3, 0) == 2 * 3 * 16

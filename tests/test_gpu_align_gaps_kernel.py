"""avsr_ctc_align_gaps, long-form CTC alignment with gap states on the blanks, against the float32
host Viterbi of tests/align_gaps_ref.py (same arithmetic, same order: exact equality, no
tolerance) and against avsr_ctc_align_long where gap_penalty = -inf makes them the same. Logits are
1e30 outside the valid columns and frames; outputs and workspace start as garbage."""
import ctypes

import numpy as np
import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import align, ops
from tests import align_gaps_ref as G
from tests import align_long_ref as R

pytestmark = pytest.mark.gpu

V, LDX = 64, 72
NINF = -float("inf")


def _labels(cases):
    B = len(cases)
    Lmax = max(1, max(len(y) for _, y in cases))
    lab = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, (_, y) in enumerate(cases):
        lab[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
    return lab, torch.tensor([len(y) for _, y in cases], dtype=torch.int32), \
        torch.tensor([Tb for Tb, _ in cases], dtype=torch.int32)


def _gap_tensor(cases, gaps, Lmax):
    """(B, Lmax + 1) uint8; positions past a row's own L + 1 flags are set: they must not be read"""
    g = torch.full((len(cases), Lmax + 1), 1, dtype=torch.uint8)
    for b, (_, y) in enumerate(cases):
        g[b, :len(y) + 1] = torch.from_numpy(np.asarray(gaps[b], dtype=np.uint8))
    return g


def _filler(x, lse, V=V):
    return (x.float()[:, :V].amax(1) - lse).contiguous()


def _launch(dev, x, lse, fil, cases, gaps, pen, T, V=V, blank=0, ws_shift=0, plain=False):
    """ops.ctc_align_gaps (plain: ops.ctc_align_long) with outputs and workspace pre-filled with
    garbage: every element must be written, none may be read"""
    B = len(cases)
    lab, llen, ilen = _labels(cases)
    ali = torch.full((B, T), 7777, dtype=torch.int32, device=dev)
    score = torch.full((B,), 7777.0, device=dev)
    feas = torch.full((B,), 7777, dtype=torch.int32, device=dev)
    nbytes = max(16, ops.ctc_align_long_ws(B, T, lab.shape[1]))
    ws = torch.full((nbytes + 16,), 255, dtype=torch.uint8, device=dev)[ws_shift:ws_shift + nbytes]
    args = (x.to(dev), B, T, V, lab.to(dev), llen.to(dev), ilen.to(dev), lse.to(dev))
    kw = dict(blank=blank, ali=ali, score=score, feasible=feas, ws=ws)
    if plain:
        ops.ctc_align_long(*args, **kw)
    else:
        ops.ctc_align_gaps(*args, _gap_tensor(cases, gaps, lab.shape[1]).to(dev), fil.to(dev), pen, **kw)
    return ali.cpu(), score.cpu(), feas.cpu()


def _reference(x, lse, fil, cases, gaps, pen, T, blank=0):
    ali, score, feas = G.align_batch(x.float().numpy(), lse.numpy(), fil.numpy(), [y for _, y in cases], gaps, pen,
                                     [Tb for Tb, _ in cases], T, blank)
    return torch.from_numpy(ali), torch.from_numpy(score), torch.from_numpy(feas)


def _same(got, want):
    """ali equal, score bit-equal, feasible equal"""
    assert torch.equal(got[2], want[2]), (got[2], want[2])
    assert torch.equal(got[0], want[0]), (got[0] != want[0]).nonzero()[:8]
    assert got[1].dtype == want[1].dtype == torch.float32
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (got[1], want[1])


def _check(dev, cases, gaps, T, pen=-0.5, dtype=torch.float32, V=V, ldx=LDX, **kw):
    x, lse = R.inputs(cases, T, V, ldx, dtype, **kw)
    fil = _filler(x, lse, V)
    got = _launch(dev, x, lse, fil, cases, gaps, pen, T, V=V)
    _same(got, _reference(x, lse, fil, cases, gaps, pen, T))
    return got


def _is_alignment_of(ali, cases):
    """a CTC path of y once GAP reads as blank"""
    for b, (Tb, y) in enumerate(cases):
        a = ali[b, :Tb].clone()
        a[a == G.GAP] = 0
        assert [sp.token for sp in align.token_spans(a)] == list(y)
        assert (ali[b, max(Tb, 0):] == -1).all()


def _ends(y):
    return G.flags_at(len(y), (0, len(y)))


# ---------------------------------------------------------------- the shared launches
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("launch", R.launches(), ids=lambda l: l[0])
def test_shared_launches(dev, launch, dtype):
    """ragged; infeasible rows between feasible ones; S = 261 and S = 1023; all ties. Random flags
    (p = 0.3, positions 0 and L included) and gap_penalty = -0.5: equal to the host reference. The
    same flags, and all flags, with -inf: equal to ops.ctc_align_long"""
    _, cases, T, kw = launch
    x, lse = R.inputs(cases, T, V, LDX, dtype, **kw)
    fil = _filler(x, lse)
    gaps = [G.random_flags(len(y), 100 + b) for b, (_, y) in enumerate(cases)]
    got = _launch(dev, x, lse, fil, cases, gaps, -0.5, T)
    _same(got, _reference(x, lse, fil, cases, gaps, -0.5, T))
    plain = _launch(dev, x, lse, fil, cases, gaps, 0.0, T, plain=True)
    _same(_launch(dev, x, lse, fil, cases, gaps, NINF, T), plain)
    _same(_launch(dev, x, lse, fil, cases, [np.ones(len(y) + 1, np.uint8) for _, y in cases], NINF, T), plain)
    _same(_launch(dev, x, lse, fil, cases, [np.zeros(len(y) + 1, np.uint8) for _, y in cases], -0.5, T), plain)


# ---------------------------------------------------------------- layout edges
@pytest.mark.parametrize("L_", [2047, 2048, 4095, 4096, 8191, 8192])
def test_layout_edges(dev, L_):
    """the recipe of tests/test_gpu_align_long_kernel.py: both sides of the P = 4 | 8 | 16 | 32
    edges (a byte / ushort / dword / two dwords of pointers per thread and frame; prefetch depth 4,
    and 1 at P = 32), T = L + adjacent repeats + 50 made odd; at L = 2048 state S - 1 = 4096 is
    alone on thread 512. Flags at 0, L and every 7th position, and at the positions of thread 3's
    first and last even state (3 P/2 and 3 P/2 + P/2 - 1): bit 0 and bit P/2 - 1 of its mask."""
    y = list(R.random_labels(L_, L_, repeats=(3, 4, L_ // 2, L_ - 2)))
    i = 10
    while (L_ + R.n_repeats(y) + 50) % 2 == 0:
        y[i + 1] = y[i]
        i += 3
    y = tuple(y)
    T = L_ + R.n_repeats(y) + 50
    assert T % 2 == 1
    S = 2 * L_ + 1
    P = 4 if S <= 4096 else 8 if S <= 8192 else 16 if S <= 16384 else 32
    H = P // 2
    g = G.flags_at(L_, list(range(0, L_ + 1, 7)) + [L_, 3 * H, 3 * H + H - 1])
    cases = [(T, y)]
    ali, _, feas = _check(dev, cases, [g], T, seed=L_)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)
    assert (ali == G.GAP).any()


# ---------------------------------------------------------------- short T
def test_short_recordings(dev):
    """T = 1 (no pointer row at all) and T = 2, 3, 5, 6, 7 around the prefetch depth, both ends
    free"""
    for T, y in ((1, (4,)), (1, ()), (2, (4,)), (3, (4, 9)), (5, (4, 4, 9)), (6, (1, 2, 3)), (7, (1, 1, 1, 1))):
        ali, _, feas = _check(dev, [(T, y)], [_ends(y)], T, seed=T)
        assert feas.tolist() == [1]
        _is_alignment_of(ali, [(T, y)])


def test_one_frame_no_labels_is_gap_or_blank_by_the_strict_compare(dev):
    x = torch.zeros(1, LDX)
    x[:, V:] = R.BIG
    x[0, 9] = 3.0
    lse = torch.logsumexp(x[:, :V], -1)
    cases, g = [(1, ())], [np.ones(1, np.uint8)]
    fil = _filler(x, lse)
    for pen, want in ((0.0, G.GAP), (-0.5, G.GAP), (-4.0, 0), (NINF, 0)):
        got = _launch(dev, x, lse, fil, cases, g, pen, 1)
        _same(got, _reference(x, lse, fil, cases, g, pen, 1))
        assert got[0].tolist() == [[want]], pen
    x[0, 0] = 3.0                                                   # the blank is the row maximum: a tie at 0
    lse = torch.logsumexp(x[:, :V], -1)
    fil = _filler(x, lse)
    got = _launch(dev, x, lse, fil, cases, g, 0.0, 1)
    _same(got, _reference(x, lse, fil, cases, g, 0.0, 1))
    assert got[0].tolist() == [[0]]


# ---------------------------------------------------------------- ties
def test_ties_at_size(dev):
    """lse = 0, logits and filler multiples of 0.5, gap_penalty = 0: path sums are exact, thousands
    of paths tie exactly, the first-maximum rule decides, and ef == eb (wherever the blank is the
    row maximum) picks the blank"""
    y = R.random_labels(1200, 17, repeats=(10, 600))
    cases = [(1500, y)]
    x, _ = R.inputs(cases, 1500, V, LDX, torch.float32, seed=18, quant=0.5)
    lse = torch.zeros(1500)
    fil = _filler(x, lse)
    g = [G.random_flags(1200, 19)]
    got = _launch(dev, x, lse, fil, cases, g, 0.0, 1500)
    _same(got, _reference(x, lse, fil, cases, g, 0.0, 1500))
    assert got[2].tolist() == [1]
    tie = fil == x[:, 0]
    assert tie.any() and (got[0][0][tie] != G.GAP).all() and (got[0][0] == G.GAP).any()


# ---------------------------------------------------------------- planted
def _planted_inputs(case, V_=V, ldx=LDX, dtype=torch.float32):
    x64, _, _, truth = G.planted(case["segments"], case["T"], case["seed"], V=V_)
    x = torch.full((case["T"], ldx), R.BIG)
    x[:, :V_] = torch.from_numpy(x64)
    x = x.to(dtype)
    lse = torch.logsumexp(x.float()[:, :V_], -1)
    return x, lse, _filler(x, lse, V_), truth


@pytest.mark.parametrize("case", [G.FREE_ENDS, G.MID_GAP], ids=["free-ends", "mid-gap"])
def test_planted(dev, case):
    """a transcript inside a longer recording, and two halves with untranscribed speech between
    them: equal to the reference, and every token on its three planted frames"""
    T, y = case["T"], case["y"]
    x, lse, fil, truth = _planted_inputs(case)
    cases, g = [(T, y)], [G.flags_at(len(y), case["flags"])]
    got = _launch(dev, x, lse, fil, cases, g, -1.0, T)
    _same(got, _reference(x, lse, fil, cases, g, -1.0, T))
    a = got[0][0].numpy()
    for i, k in enumerate(y):
        assert np.nonzero(a == k)[0].tolist() == list(range(*truth[i])), (i, k)
    if case is G.FREE_ENDS:
        assert np.nonzero(a > 0)[0][0] == 40 and np.nonzero(a > 0)[0][-1] < 80 and (a == G.GAP).sum() == 80


def test_planted_full_vocabulary_bf16(dev):
    """the model's V = 5049 / ldx = 5056 in bf16"""
    case = G.FREE_ENDS
    T, y = case["T"], case["y"]
    x, lse, fil, truth = _planted_inputs(case, 5049, 5056, torch.bfloat16)
    cases, g = [(T, y)], [G.flags_at(len(y), case["flags"])]
    got = _launch(dev, x, lse, fil, cases, g, -1.0, T, V=5049)
    _same(got, _reference(x, lse, fil, cases, g, -1.0, T))
    a = got[0][0].numpy()
    assert np.nonzero(a > 0)[0][0] == 40 and np.nonzero(a > 0)[0][-1] < 80


# ---------------------------------------------------------------- batch
def test_batch_rows_equal_their_own_launch(dev):
    """B = 3, T padded to 700: different in_len and label_len, one infeasible row (fewer frames
    than labels), one with L = 0 and a free start; Lmax = 600 for all of them"""
    T = 700
    cases = [(650, R.random_labels(600, 20, repeats=(7,))), (90, R.random_labels(100, 21)), (333, ())]
    gaps = [G.random_flags(600, 25), G.random_flags(100, 26), np.ones(1, np.uint8)]
    x, lse = R.inputs(cases, T, V, LDX, torch.float32, seed=22)
    fil = _filler(x, lse)
    got = _launch(dev, x, lse, fil, cases, gaps, -0.5, T)
    _same(got, _reference(x, lse, fil, cases, gaps, -0.5, T))
    assert got[2].tolist() == [1, 0, 1]
    assert got[0][1].tolist() == [-1] * T and got[1][1].item() == 0.0
    assert set(got[0][2][:333].tolist()) <= {0, G.GAP} and got[0][2][333:].tolist() == [-1] * (T - 333)
    for b in range(3):
        r = slice(b * T, (b + 1) * T)
        alone = _launch(dev, x[r], lse[r], fil[r], cases[b:b + 1], gaps[b:b + 1], -0.5, T)
        _same(alone, tuple(o[b:b + 1] for o in got))


# ---------------------------------------------------------------- errors
def test_argument_errors(dev):
    cases = [(25, R.Y6)]
    x, lse = R.inputs(cases, 25, V, LDX, torch.float32)
    fil = _filler(x, lse)
    g = [_ends(R.Y6)]
    _launch(dev, x, lse, fil, cases, g, -0.5, 25)
    for pen in (0.1, float("nan")):
        with pytest.raises(L.AvsrLibError, match="1004"):        # AVSR_E_ARG
            _launch(dev, x, lse, fil, cases, g, pen, 25)
    for shift in (1, 4, 8):
        with pytest.raises(L.AvsrLibError, match="1002"):        # AVSR_E_ALIGN
            _launch(dev, x, lse, fil, cases, g, -0.5, 25, ws_shift=shift)
    y = R.random_labels(16384, 15)
    with pytest.raises(L.AvsrLibError, match="1001"):            # AVSR_E_SHAPE
        _launch(dev, x, lse, fil, [(25, y)], [_ends(y)], -0.5, 25)
    # gap or filler NULL
    lab, llen, ilen = _labels(cases)
    t = dict(x=x.to(dev), lse=lse.to(dev), labels=lab.to(dev), label_len=llen.to(dev), in_len=ilen.to(dev),
             ws=torch.empty(ops.ctc_align_long_ws(1, 25, 6), dtype=torch.uint8, device=dev),
             ali=torch.empty(1, 25, dtype=torch.int32, device=dev), score=torch.empty(1, device=dev),
             feasible=torch.empty(1, dtype=torch.int32, device=dev))
    for missing in ("gap", "filler"):
        more = dict(gap=_gap_tensor(cases, g, 6).to(dev), filler=fil.to(dev))
        more[missing] = None
        p = L.fill(L.CtcAlignGapsParams, dtype=L.AVSR_F32, B=1, T=25, V=V, Lmax=6, blank=0, ldx=LDX, gap_penalty=-0.5,
                   **t, **more)
        assert L.load().avsr_ctc_align_gaps(ctypes.byref(p), L.stream_ptr()) == 1004, missing
    # the Python layer's own checks
    d = [a.to(dev) for a in (x, lab, llen, ilen, lse)]

    def call(gap, filler):
        return ops.ctc_align_gaps(d[0], 1, 25, V, d[1], d[2], d[3], d[4], gap, filler, -0.5)

    with pytest.raises(TypeError):
        call(more["gap"].to(torch.int32), fil.to(dev))
    with pytest.raises(TypeError):
        call(_gap_tensor(cases, g, 6).to(dev), fil.double().to(dev))
    with pytest.raises(ValueError):
        call(torch.zeros(1, 6, dtype=torch.uint8, device=dev), fil.to(dev))
    with pytest.raises(ValueError):
        call(_gap_tensor(cases, g, 6).to(dev), fil[:24].to(dev))


# ---------------------------------------------------------------- the bound
def test_the_bound(dev):
    """L = 16383 (S = 32767, P = 32), T = 16500, both ends free: a CTC path of y once GAP reads as
    blank, whose score is the gap-aware sequential float32 sum along it, bit for bit
    (tests/test_align_gaps_ref.py: that is what the score is); optimality is what the smaller cases
    establish"""
    T, Tp = 16500, 16520
    y = R.random_labels(16383, 15, distinct=True)
    cases = [(T, y)]
    x, lse = R.inputs(cases, Tp, V, LDX, torch.float32, seed=16)
    fil = _filler(x, lse)
    ali, score, feas = _launch(dev, x, lse, fil, cases, [_ends(y)], -0.5, Tp)
    assert feas.tolist() == [1]
    _is_alignment_of(ali, cases)
    assert (ali[0, :T] == G.GAP).any()
    want = G.path_sum(x.numpy(), lse.numpy(), fil.numpy(), -0.5, ali[0, :T].numpy())
    assert score.numpy()[0].view(np.int32) == want.view(np.int32), (score, want)

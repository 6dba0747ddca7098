"""avsr_ctc_kws on the device against the float32 numpy DP of tests/kws_ref.py (same arithmetic,
same order: exact equality, score as bit patterns, no pair exempt). Inputs are randn * 3 logits
through ops.log_softmax_topk; everything the kernel must not read (columns >= V, frames >=
tlen[u], labels beyond a keyword's length) holds a value that would show, and every output starts
as 7777."""
import ctypes

import numpy as np
import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import ops
from tests import kws_ref as R

pytestmark = pytest.mark.gpu

BIG = 1e30
V, LDP = 64, 72
Y6 = (5, 17, 30, 42, 40, 9)
KEYWORDS = [(11,), (7, 47), Y6, (7, 7, 7, 3, 3), (9, 9, 9, 9), (4,), (1, 2), (63, 1, 63), (33, 33)]   # K = 9
Y32 = tuple(1 + (7 * i) % 63 for i in range(32))                                        # S = 63, no repeats


def _inputs(dev, tlens, Tm, seed=0, const=None):
    """logp (U, Tm, LDP)[..., :V] view and top (U, Tm) from the device's log-softmax + argmax of
    random (or constant) logits, then BIG in every column >= V and every frame >= tlen[u]"""
    U = len(tlens)
    if const is None:
        x = torch.randn(U * Tm, V, generator=torch.Generator().manual_seed(seed)) * 3
    else:
        x = torch.full((U * Tm, V), float(const))
    buf = torch.full((U, Tm, LDP), BIG, device=dev)
    top = torch.empty(U, Tm, dtype=torch.int32, device=dev)
    ops.log_softmax_topk(x.to(dev), V, buf.view(U * Tm, LDP), 1, top.view(U * Tm, 1))
    for u, n in enumerate(tlens):
        buf[u, max(min(n, Tm), 0):] = BIG
    assert (buf[..., V:] == BIG).all()
    return buf[..., :V], top


def _launch(dev, logp, top, tlens, kws, trace=True, blank=0, Lmax=None):
    U, Tm = logp.shape[:2]
    K = len(kws)
    Lmax = max(len(y) for y in kws) if Lmax is None else Lmax
    lab = torch.full((K, Lmax), 1 << 20, dtype=torch.int32)              # an id far outside [0, V)
    for k, y in enumerate(kws):
        lab[k, :len(y)] = torch.tensor(y, dtype=torch.int32)
    out = dict(score=torch.full((U, K), 7777.0, device=dev), start=torch.full((U, K), 7777, dtype=torch.int32, device=dev),
               end=torch.full((U, K), 7777, dtype=torch.int32, device=dev))
    if trace:
        out.update(trace_out=torch.full((U, K, Tm), 7777.0, device=dev),
                   tstart_out=torch.full((U, K, Tm), 7777, dtype=torch.int32, device=dev))
    got = ops.ctc_kws(logp, torch.tensor(tlens, dtype=torch.int32).to(dev), top, lab.to(dev),
                      torch.tensor([len(y) for y in kws], dtype=torch.int32).to(dev), blank=blank, **out)
    return tuple(t.cpu() for t in got)


def _reference(logp, top, tlens, kws, blank=0):
    want = R.spot_batch(logp.cpu().numpy(), tlens, None if top is None else top.cpu().numpy(), kws, blank, V=V, Lmax=32)
    return tuple(torch.from_numpy(w) for w in want)


def _same(got, want):
    """score (and trace) bit-equal, start / end (and tstart) equal"""
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), (g != w).nonzero()[:8]


@pytest.fixture(scope="module")
def ragged(dev):
    tlens = [40, 17, 1]
    logp, top = _inputs(dev, tlens, 40)
    return tlens, logp, top, _reference(logp, top, tlens, KEYWORDS), _reference(logp, None, tlens, KEYWORDS)


@pytest.mark.parametrize("filler", [True, False])
def test_ragged_launch(dev, ragged, filler):
    """U = 3 of 40 / 17 / 1 frames, K = 9 (a tail block of one wave): lengths 1, 2, 6, repeats, a
    keyword that fits only the longest utterance; with the filler and without"""
    tlens, logp, top, want_f, want_n = ragged
    want = want_f if filler else want_n
    got = _launch(dev, logp, top if filler else None, tlens, KEYWORDS, trace=False)
    _same(got, want[:3])
    score, start, end = got
    assert torch.isfinite(score[0]).all() and (start[0] >= 0).all() and (end[0] > start[0]).all()
    assert score[1, 4] > -np.inf and score[2, 4] == -np.inf             # (9, 9, 9, 9) needs 7 frames
    assert torch.isfinite(score[2]).tolist() == [len(y) == 1 for y in KEYWORDS]
    assert (start[2][torch.isfinite(score[2])] == 0).all() and (end[2][torch.isfinite(score[2])] == 1).all()
    if filler:
        assert (score <= 0).all()


@pytest.mark.parametrize("filler", [True, False])
def test_traces(dev, ragged, filler):
    """trace / tstart equal the reference at every frame, -inf / -1 beyond tlen; score / start /
    end are the same with traces as without"""
    tlens, logp, top, want_f, want_n = ragged
    want = want_f if filler else want_n
    got = _launch(dev, logp, top if filler else None, tlens, KEYWORDS, trace=True)
    _same(got, want)
    trace, tstart = got[3], got[4]
    for u, n in enumerate(tlens):
        assert (trace[u, :, n:] == -np.inf).all() and (tstart[u, :, n:] == -1).all()
    assert (trace[0, 0] > -np.inf).all()                                # one piece: an occurrence ends at every frame


@pytest.mark.parametrize("filler", [True, False])
def test_widest_keyword(dev, filler):
    """32 pieces, S = 63 states (the bound), Tm = 70 (nine blocks of frames, the last partial),
    next to a one-piece keyword in the same launch"""
    tlens = [70, 33, 31]
    logp, top = _inputs(dev, tlens, 70, seed=1)
    kws = [Y32, (5,), Y32[:31]]
    got = _launch(dev, logp, top if filler else None, tlens, kws)
    _same(got, _reference(logp, top if filler else None, tlens, kws))
    assert torch.isfinite(got[0]).tolist() == [[True] * 3, [True] * 3, [False, True, True]]


@pytest.mark.parametrize("const", [0.0, -1.7])
def test_all_ties(dev, const):
    """constant logits: every cell ties; the span is the whole utterance, score 0"""
    tlens = [9, 23, 4]
    logp, top = _inputs(dev, tlens, 23, const=const)
    kws = [(3,), (3, 3, 5), (5, 1, 5, 5), Y6]
    got = _launch(dev, logp, top, tlens, kws)
    _same(got, _reference(logp, top, tlens, kws))
    score, start, end = got[:3]
    for u, n in enumerate(tlens):
        for k, y in enumerate(kws):
            fits = n >= len(y) + sum(a == b for a, b in zip(y, y[1:]))
            assert (score[u, k].item(), start[u, k].item(), end[u, k].item()) == ((0.0, 0, n) if fits else (-np.inf, -1, -1))


def test_infeasible_between_feasible(dev):
    """utterances of 0 frames and of more than Tm frames (read as Tm), keywords that are too long
    for some utterances, a label outside [0, V), a blank inside a keyword: -inf / -1 / -1 there,
    and every feasible pair equals its result when launched alone (K = 1, U = 1)"""
    Tm = 25
    tlens = [12, 0, 25, 3, 99, 7]
    logp, top = _inputs(dev, [min(n, Tm) for n in tlens], Tm, seed=2)
    kws = [(7, 7, 7, 3, 3), (9, 9, 9, 9), (7, 64, 3), Y6, (1, 2, 3, 4), (4, 0, 5), (-1, 2), (8,)]
    got = _launch(dev, logp, top, tlens, kws)
    ref_len = [min(n, Tm) for n in tlens]
    _same(got, _reference(logp, top, ref_len, kws))
    score, start, end, trace, tstart = got
    feas = torch.isfinite(score)
    assert feas.tolist() == [[min(n, Tm) >= len(y) + sum(a == b for a, b in zip(y, y[1:])) and k not in (2, 5, 6)
                              for k, y in enumerate(kws)] for n in tlens]
    assert (start[~feas] == -1).all() and (end[~feas] == -1).all()
    assert (trace[~feas] == -np.inf).all() and (tstart[~feas] == -1).all()
    for u, k in feas.nonzero().tolist():
        alone = _launch(dev, logp[u:u + 1], top[u:u + 1], tlens[u:u + 1], kws[k:k + 1])
        _same(alone, tuple(o[u:u + 1, k:k + 1] for o in got))


def test_other_blank(dev):
    tlens = [20, 11]
    logp, top = _inputs(dev, tlens, 20, seed=3)
    kws = [(7, 7, 0, 3), (1, 2), (5, 6)]                                # blank = 5: the last one is refused
    got = _launch(dev, logp, top, tlens, kws, blank=5)
    _same(got, _reference(logp, top, tlens, kws, blank=5))
    assert torch.isfinite(got[0]).tolist() == [[True, True, False]] * 2


def test_error_codes(dev):
    tlens = [12]
    logp, top = _inputs(dev, tlens, 12, seed=4)
    with pytest.raises(L.AvsrLibError, match="1001"):                    # AVSR_E_SHAPE: Lmax = 33
        _launch(dev, logp, top, tlens, [(1, 2)], Lmax=33)
    lib = L.load()
    assert lib.avsr_ctc_kws(None, None) == 1004                          # AVSR_E_ARG: no params
    lab = torch.tensor([[1, 2]], dtype=torch.int32, device=dev)
    llen = torch.tensor([2], dtype=torch.int32, device=dev)
    tl = torch.tensor(tlens, dtype=torch.int32, device=dev)
    with pytest.raises(L.AvsrLibError, match="1004"):                    # trace without tstart
        ops.ctc_kws(logp, tl, top, lab, llen, blank=0, trace_out=torch.empty(1, 1, 12, device=dev))
    with pytest.raises(L.AvsrLibError, match="1004"):                    # and the reverse
        ops.ctc_kws(logp, tl, top, lab, llen, blank=0, tstart_out=torch.empty(1, 1, 12, dtype=torch.int32, device=dev))
    p = L.fill(L.CtcKwsParams, U=1, Tm=12, V=V, K=1, Lmax=2, blank=0, logp=logp, ldp=LDP, tlen=tl, top=top,
               labels=lab, label_len=llen)                               # no outputs
    assert lib.avsr_ctc_kws(ctypes.byref(p), L.stream_ptr()) == 1004
    for field in ("U", "K", "Tm", "Lmax"):                               # AVSR_E_SHAPE: a size of 0
        p = L.fill(L.CtcKwsParams, **{**dict(U=1, Tm=12, V=V, K=1, Lmax=2), field: 0})
        assert lib.avsr_ctc_kws(ctypes.byref(p), L.stream_ptr()) == 1001, field
    torch.cuda.synchronize()

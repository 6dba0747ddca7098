"""avsr_amd.longform.align_partial on the device. The tiny golden model of tests/test_gpu_longform.py
serves as `e2e` only; the logits are the planted (T, Vp) tensors of tests/align_gaps_ref.py in the
engine dtype with lse from ops.row_lse, so nothing depends on random weights: the planted frames
are recovered, everything equals the host reference, and with no gap state it is align_long."""
import numpy as np
import pytest
import torch

from avsr_amd import align, longform, ops
from avsr_amd.avhubert_avsr_model import AVHubertAVSR
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests import align_gaps_ref as G
from tests.oracle_util import golden_state, load_golden

pytestmark = pytest.mark.gpu

PEN = -1.0


@pytest.fixture(scope="module")
def e2e(dev):
    st = golden_state(load_golden())
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    m.setup_engine("cuda", torch.float32)
    return m.eval().avsr


@pytest.fixture(scope="module")
def recs(e2e):
    """per planted case: device logits (T, Vp) and lse, their host copies and the host filler
    (computed once, read-only)"""
    eng = e2e.engine()
    out = {}
    for name, case in (("free-ends", G.FREE_ENDS), ("mid-gap", G.MID_GAP)):
        x, _, _, truth = G.planted(case["segments"], case["T"], case["seed"], V=eng.V)
        logits = torch.full((case["T"], eng.Vp), 1e30)
        logits[:, :eng.V] = torch.from_numpy(x)
        logits = logits.to(eng.device, eng.dtype)
        lse = ops.row_lse(logits, eng.V, torch.empty(case["T"], device=eng.device))
        xh, lh = logits.float().cpu().numpy(), lse.cpu().numpy()
        out[name] = dict(case=case, logits=logits, lse=lse, x=xh, l=lh, fil=G.filler_of(xh, lh, eng.V), truth=truth)
    return out


def _bits(v):
    return np.float32(v).view(np.int32)


@pytest.mark.parametrize("name", ["free-ends", "mid-gap"])
def test_align_partial_recovers_the_planted_frames(e2e, recs, name):
    r = recs[name]
    case, T = r["case"], r["case"]["T"]
    y = list(case["y"])
    inner = [i for i in case["flags"] if 0 < i < len(y)]
    a = longform.align_partial(e2e, r["logits"], r["lse"], [e2e.sos] + y + [e2e.eos], gap_penalty=PEN, gaps=inner)
    assert [sp.token for sp in a.spans] == y
    assert [(sp.start, sp.end) for sp in a.spans] == [r["truth"][i] for i in range(len(y))]
    # the host reference on the same logits
    ali, score, feas = G.viterbi(r["x"], r["l"], r["fil"], y, G.flags_at(len(y), case["flags"]), PEN, T, e2e.blank)
    assert feas == 1 and a.ali.dtype == np.int32 and np.array_equal(a.ali, ali)
    assert _bits(a.score) == _bits(score), (a.score, score)
    assert a.frame_logp.dtype == np.float32
    assert np.array_equal(a.frame_logp, G.frame_terms(r["x"], r["l"], r["fil"], PEN, ali))
    acc = a.frame_logp[0]
    for v in a.frame_logp[1:]:
        acc = np.float32(acc + v)
    assert _bits(acc) == _bits(score)
    assert a.spans == align.token_spans(np.where(ali == G.GAP, e2e.blank, ali), e2e.blank)
    # gaps are the maximal runs of -2
    assert [tuple(g) for g in a.gaps] == G.gap_runs(ali) == longform.uncovered(a) and len(a.gaps) >= 2
    assert sum(b - lo for lo, b in a.gaps) == int((ali == G.GAP).sum())
    # clips stay out of them, and hold every token once
    token_list = ["▁w%d" % i for i in range(e2e.engine().V)]
    segs = longform.segments(a, token_list, max_frames=375)
    assert [t for s in segs for t in s.tokens] == y
    for s in segs:
        assert not (a.ali[s.start:s.end] == G.GAP).any()
    assert len(segs) == (2 if name == "mid-gap" else 1)


def test_no_gap_state_is_align_long(e2e, recs):
    r = recs["mid-gap"]
    y = list(r["case"]["y"])
    want = longform.align_long(e2e, r["logits"], r["lse"], y)
    for kw in (dict(gap_penalty=PEN, free_start=False, free_end=False, gaps=()),
               dict(gap_penalty=-float("inf"), gaps="all")):
        a = longform.align_partial(e2e, r["logits"], r["lse"], y, **kw)
        assert a.spans == want.spans and a.score == want.score
        assert a.frame_logp.dtype == want.frame_logp.dtype and np.array_equal(a.frame_logp, want.frame_logp)
        assert a.gaps == [] and not (a.ali == G.GAP).any()
        assert align.token_spans(a.ali, e2e.blank) == want.spans


def test_none_where_no_alignment_exists(e2e, recs):
    r = recs["free-ends"]
    T = r["case"]["T"]
    kw = dict(gap_penalty=PEN, gaps="all")
    assert longform.align_partial(e2e, r["logits"], r["lse"], [1 + i % 7 for i in range(T + 1)], **kw) is None
    assert longform.align_partial(e2e, r["logits"], r["lse"], [9] * (T // 2 + 1), **kw) is None      # L + repeats > T
    assert longform.align_partial(e2e, r["logits"], r["lse"], [9] * (T // 2), **kw) is not None

"""avsr_amd.longform on the tiny golden model: the CTC logits of a 100-frame "recording" encoded in
overlapping 40-frame windows are bit-equal to doing the documented grouping by hand; the
alignment of its greedy transcript equals the host reference on those logits; the clips hold
every token once."""
import numpy as np
import pytest
import torch

from avsr_amd import align, longform, ops
from avsr_amd.avhubert_avsr_model import AVHubertAVSR
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests import align_long_ref as R
from tests.oracle_util import golden_state, load_golden

pytestmark = pytest.mark.gpu

T = 100
SEED = 0


@pytest.fixture(scope="module")
def e2e(dev):
    st = golden_state(load_golden())
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    m.setup_engine("cuda", torch.float32)
    return m.eval().avsr


@pytest.fixture(scope="module")
def rec(e2e):
    """the recording, its stitched logits and lse (computed once, read-only), and its greedy
    transcript: the collapse of the frame-wise best non-eos token, a CTC path by construction"""
    g = torch.Generator().manual_seed(SEED)
    videos, audios = torch.randn(1, 1, T, 88, 88, generator=g), torch.randn(1, 104, T, generator=g)
    logits, lse = longform.ctc_logits_long(e2e, videos, audios, window=40, overlap=16, batch=2)
    V = e2e.engine().V
    best = logits[:, :V].clone()
    best[:, e2e.eos] = -float("inf")
    y = [sp.token for sp in align.token_spans(best.argmax(-1).cpu().numpy(), e2e.blank)]
    return dict(videos=videos, audios=audios, logits=logits, lse=lse, y=y)


def _head(eng, x):
    """the CTC head over the rows of one window: one GEMM launch"""
    cl = torch.zeros(x.shape[0], eng.Vp, device=eng.device, dtype=eng.dtype)
    ops.linear_fwd(x.contiguous(), eng.w("ctc.ctc_lo.weight"), eng.arena.master("ctc.ctc_lo.bias"), out=cl[:, :eng.V])
    return cl


def test_ctc_logits_long_is_the_documented_grouping(e2e, rec):
    eng = e2e.engine()
    plan = longform.window_plan(T, 40, 16)
    assert len(plan) == 4                       # two groups of two windows
    want = torch.zeros(T, eng.Vp, device=eng.device, dtype=eng.dtype)
    for g in (0, 2):
        grp = plan[g:g + 2]
        vid = torch.cat([rec["videos"][:, :, s:e] for s, e, _, _ in grp], 0)
        aud = torch.cat([rec["audios"][:, :, s:e] for s, e, _, _ in grp], 0)
        enc = eng.encode(aud, vid, torch.full((2,), 40, dtype=torch.int64))
        assert enc.dtype == eng.dtype
        for i, (s, e, lo, hi) in enumerate(grp):
            want[lo:hi] = _head(eng, enc[i])[lo - s:hi - s]
    logits, lse = rec["logits"], rec["lse"]
    assert logits.shape == (T, eng.Vp) and logits.dtype == eng.dtype and logits.device.type == "cuda"
    assert torch.equal(logits, want)
    assert lse.shape == (T,) and lse.dtype == torch.float32
    assert torch.equal(lse, ops.row_lse(want, eng.V, torch.empty(T, device=eng.device)))
    # a device-resident recording gives the same
    again, _ = longform.ctc_logits_long(e2e, rec["videos"].cuda(), rec["audios"].cuda(), window=40, overlap=16, batch=2)
    assert torch.equal(again, want)


def test_one_window_is_engine_encode(e2e, rec):
    eng = e2e.engine()
    logits, lse = longform.ctc_logits_long(e2e, rec["videos"], rec["audios"], window=375)
    enc = eng.encode(rec["audios"], rec["videos"], torch.tensor([T]))
    want = _head(eng, enc[0])
    assert torch.equal(logits, want)
    assert torch.equal(lse, ops.row_lse(want, eng.V, torch.empty(T, device=eng.device)))


def test_align_long_and_segments(e2e, rec):
    y, logits, lse = rec["y"], rec["logits"], rec["lse"]
    assert len(y) >= 5, y
    a = longform.align_long(e2e, logits, lse, y)
    assert [sp.token for sp in a.spans] == y
    x, l = logits.float().cpu().numpy(), lse.cpu().numpy()
    ali, score, feas = R.viterbi(x, l, y, T, e2e.blank)
    assert feas == 1 and a.spans == align.token_spans(ali, e2e.blank)
    assert np.float32(a.score).view(np.int32) == score.view(np.int32), (a.score, score)
    assert a.frame_logp.dtype == np.float32 and a.frame_logp.shape == (T,)
    assert np.array_equal(a.frame_logp, x[np.arange(T), ali] - l)
    acc = a.frame_logp[0]
    for v in a.frame_logp[1:]:
        acc = np.float32(acc + v)
    assert acc.view(np.int32) == score.view(np.int32)
    # sos / eos at the ends are stripped
    b = longform.align_long(e2e, logits, lse, [e2e.sos] + y + [e2e.eos])
    assert b.spans == a.spans and b.score == a.score
    # clips: every token once, in order; a clip of several words fits
    token_list = [("▁w%d" if i % 3 == 0 else "p%d") % i for i in range(e2e.engine().V)]
    segs = longform.segments(a, token_list, max_frames=30)
    assert [t for s in segs for t in s.tokens] == y
    assert [s.first for s in segs] == [0] + [s.last + 1 for s in segs[:-1]] and segs[-1].last == len(y) - 1
    for s in segs:
        assert 0 <= s.start < s.end <= T and s.worst <= 0.0 and s.score <= 0.0
        assert s.end - s.start <= 30 or len(s.text.split()) == 1
    assert [s.start for s in segs] == sorted(s.start for s in segs)
    assert all(p.end <= q.start for p, q in zip(segs, segs[1:]))


def test_align_long_infeasible_and_errors(e2e, rec):
    logits, lse = rec["logits"], rec["lse"]
    V = e2e.engine().V
    assert longform.align_long(e2e, logits, lse, [1 + i % 7 for i in range(T + 1)]) is None     # more tokens than frames
    assert longform.align_long(e2e, logits, lse, [9] * 51) is None                                 # 51 + 50 repeats > 100
    for bad in ([3, V, 4], [3, -1], [3, e2e.blank, 4], [3, e2e.eos, 4], [1 + i % 7 for i in range(16384)]):
        with pytest.raises(ValueError):
            longform.align_long(e2e, logits, lse, bad)

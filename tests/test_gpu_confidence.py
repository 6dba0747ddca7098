"""avsr_amd.confidence on the tiny model (oracle.weights.TINY_CONFIG, golden weights, eval), fp32
engine unless a test says otherwise. Hypotheses come from the joint search (ctc_weight 0.1, beam 3)
on three utterances of different lengths, plus a short transcript over the first utterance (the
random tiny model never ends a hypothesis by itself, so the search's hypotheses have one token per
frame: the transcript is the case with frames to spare).

The CTC term is checked twice: the posterior arithmetic alone, from the kernel's own sub / del in
fp64 (1e-6: fp32 exp / log rounding on values in [0, 1]); and end to end against the fp64 reference
of tests/confidence_ref.py on the device's own CTC logits, |d conf_ctc| <= 2 * delta with delta =
the score tolerance of tests/test_gpu_ctc_neighbors.py (1e-5 fp32, 1e-3 bf16) * max |finite
reference score|: conf = exp(a - Z), and both a and Z move by at most delta."""
import math

import pytest
import torch

from avsr_amd import align, confidence, ops, rescore
from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder, get_rescoring_decoder
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests import confidence_ref as R
from tests.oracle_util import golden_state, load_golden

pytestmark = pytest.mark.gpu

V = 5049
TOKENS = ["<blank>"] + [("▁" if i % 3 == 1 else "") + f"u{i}" for i in range(1, V - 1)] + ["<eos>"]
W, K = 0.1, 4


def _model(dtype):
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT)).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(load_golden()).items()}, strict=True)
    m.setup_engine("cuda", dtype)
    return m


@pytest.fixture(scope="module")
def model(dev):
    return _model(torch.float32)


@pytest.fixture(scope="module")
def utts(model):
    """(encoded utterances, token sequences without sos / eos)"""
    g = load_golden()
    x0, x1 = (torch.from_numpy(g[f"dec_enc_{b}"]).cuda() for b in range(2))
    xs = [x0, x1, x0[:12].contiguous()]
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=W, beam_size=3)
    ys = [align.strip_sos_eos(bs(x)[0].yseq.tolist(), model.avsr.sos, model.avsr.eos) for x in xs]
    return xs + [x0], ys + [ys[0][:6]]


@pytest.fixture(scope="module")
def conf(model, utts):
    return confidence.confidence_batch(model.avsr, utts[0], utts[1], ctc_weight=W, alternatives=K)


def _device_scores(e2e, xs, ys):
    """what confidence_batch launches, copied to the host: CTC logits (per utterance, fp32 upcast),
    and the kernel's sub / del / base / feasible for the padded batch"""
    eng = e2e.engine()
    _, cl, Ts, Tm = rescore.ctc_logits(eng, xs)
    Lmax = max(1, max(len(y) for y in ys))
    lab = torch.full((len(ys), Lmax), -1, dtype=torch.int32)
    for u, y in enumerate(ys):
        lab[u, :len(y)] = torch.tensor(y, dtype=torch.int32)
    lse = torch.empty(len(xs) * Tm, device=eng.device, dtype=torch.float32)
    ops.row_lse(cl, eng.V, lse)
    sub, dele, base, feas = ops.ctc_neighbors(cl, len(xs), Tm, eng.V, lab.cuda(),
                                              torch.tensor([len(y) for y in ys], dtype=torch.int32).cuda(),
                                              torch.tensor(Ts, dtype=torch.int32).cuda(), lse, blank=e2e.blank, eos=e2e.eos)
    logits = [cl[u * Tm:u * Tm + Ts[u], :eng.V].float().cpu() for u in range(len(xs))]
    return logits, sub.cpu(), dele.cpu(), base.cpu(), feas.cpu()


@pytest.fixture(scope="module")
def scores(model, utts):
    return _device_scores(model.avsr, *utts)


@pytest.fixture(scope="module")
def reference(model, utts, scores):
    """per utterance the fp64 (sub, del, base) of the explicit neighbours on the device's own logits
    (None where y has no path); computed once"""
    out = []
    for x, y, lg in zip(utts[0], utts[1], scores[0]):
        ok = rescore.ctc_feasible(int(x.shape[0]), y)
        out.append(R.neighbors(torch.log_softmax(lg.double(), -1), y, int(x.shape[0]), model.avsr.blank, model.avsr.eos)
                   if ok else None)
    return out


def test_hypotheses_are_scored(model, utts, conf):
    assert len(conf) == 4 and conf[3] is not None
    for (x, y, c) in zip(utts[0], utts[1], conf):
        assert (c is None) == (not rescore.ctc_feasible(int(x.shape[0]), y))
        if c is None:
            continue
        assert [t.token for t in c.tokens] == y
        for t in c.tokens:
            assert 0.0 < t.ctc <= 1.0 and 0.0 < t.decoder <= 1.0 and 0.0 < t.joint <= 1.0
            assert len(t.alternatives) <= K and all(a[0] != t.token for a in t.alternatives)
            assert [a[1] for a in t.alternatives] == sorted((a[1] for a in t.alternatives), reverse=True)
            assert t.ctc + sum(a[1] for a in t.alternatives) <= 1.0 + 1e-6
        assert 0.0 < c.eos <= 1.0 and 0.0 < c.utterance <= 1.0 and c.base < 0.0


def test_posterior_arithmetic_from_kernel_scores(model, utts, conf, scores):
    """ctc, the alternatives' posteriors and their order = the fp64 posterior of the kernel's own numbers"""
    _, sub, dele, base, feas = scores
    for u, (y, c) in enumerate(zip(utts[1], conf)):
        assert bool(feas[u]) == (c is not None)
        if c is None:
            continue
        assert c.base == base[u].item()
        want = R.posteriors(sub[u, :len(y), :V], dele[u, :len(y)], y, k=K, blank=model.avsr.blank, eos=model.avsr.eos)
        for t, (p, alts) in zip(c.tokens, want):
            assert abs(t.ctc - p) <= 1e-6, (u, t, p)
            assert [a[0] for a in t.alternatives] == [a[0] for a in alts], (u, t, alts)
            assert all(abs(a[1] - b[1]) <= 1e-6 for a, b in zip(t.alternatives, alts)), (u, t, alts)


def _ctc_bound(ref, tol):
    sub, dele, base = ref
    finite = torch.cat([sub[torch.isfinite(sub)], dele[torch.isfinite(dele)], torch.tensor([base], dtype=torch.float64)])
    return 2.0 * tol * finite.abs().max().item()


def test_ctc_term_end_to_end(model, utts, conf, reference):
    for u, (y, c, ref) in enumerate(zip(utts[1], conf, reference)):
        if ref is None:
            assert c is None
            continue
        want = R.posteriors(ref[0], ref[1], y, blank=model.avsr.blank, eos=model.avsr.eos)
        bound = _ctc_bound(ref, 1e-5)
        err = max(abs(t.ctc - p) for t, (p, _) in zip(c.tokens, want))
        print(f"utt {u}: max |d conf_ctc| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (u, err, bound)
        assert abs(c.base - ref[2]) <= 1e-5 * abs(ref[2])


def test_decoder_term_is_the_rescoring_pass(model, utts, conf):
    """decoder and eos = exp of the per-target log-probs of the two-pass decoder's second pass, bit for bit"""
    search = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=W)
    for x, y, c in zip(utts[0], utts[1], conf):
        if c is None:
            continue
        lp = search.rescore(x, [y])[0].states["decoder"]
        assert lp.dtype == torch.float32 and lp.numel() == len(y) + 1
        assert [t.decoder for t in c.tokens] == [math.exp(float(v)) for v in lp[:-1]]
        assert c.eos == math.exp(float(lp[-1]))


def test_joint_and_utterance(model, utts, conf):
    for c in conf:
        if c is None:
            continue
        for t in c.tokens:
            assert t.joint == pytest.approx(math.exp((1 - W) * math.log(t.decoder) + W * math.log(t.ctc)), rel=1e-12)
        gm = math.exp(sum(math.log(t.joint) for t in c.tokens) / len(c.tokens))
        assert c.utterance == pytest.approx(gm, rel=1e-12)
    xs, ys = utts[0][3:], utts[1][3:]
    dec_only, = confidence.confidence_batch(model.avsr, xs, ys, ctc_weight=0.0, alternatives=K)
    ctc_only, = confidence.confidence_batch(model.avsr, xs, ys, ctc_weight=1.0, alternatives=K)
    both = conf[3]
    assert dec_only.base is None and ctc_only.eos is None and dec_only.eos == both.eos and ctc_only.base == both.base
    for d, c, b in zip(dec_only.tokens, ctc_only.tokens, both.tokens):
        assert d.ctc is None and d.alternatives == [] and d.decoder == b.decoder and d.joint == d.decoder
        assert c.decoder is None and c.ctc == b.ctc and c.joint == c.ctc and c.alternatives == b.alternatives
    empty, = confidence.confidence_batch(model.avsr, xs, [[]], ctc_weight=W)
    assert empty.tokens == [] and empty.utterance == 1.0 and 0.0 < empty.eos <= 1.0 and empty.base < 0.0


def test_batch_independence(model, utts, conf):
    for x, y, c in zip(utts[0], utts[1], conf):
        alone, = confidence.confidence_batch(model.avsr, [x], [y], ctc_weight=W, alternatives=K)
        assert alone == c
    sos, eos = model.avsr.sos, model.avsr.eos
    wrapped = confidence.confidence_batch(model.avsr, utts[0], [[sos] + y + [eos] for y in utts[1]], ctc_weight=W,
                                          alternatives=K)
    assert wrapped == conf


def test_infeasible_gives_none(model, utts, conf):
    xs, ys = list(utts[0]), [list(y) for y in utts[1]]
    ys[2] = [9] * 7                               # 12 frames, 7 equal labels need 13
    mixed = confidence.confidence_batch(model.avsr, xs, ys, ctc_weight=W, alternatives=K)
    assert mixed[2] is None
    assert all(m == c for i, (m, c) in enumerate(zip(mixed, conf)) if i != 2)
    xs[1], ys[1] = xs[1][:3], [5, 6, 7, 8]        # more labels than frames
    assert confidence.confidence_batch(model.avsr, xs, ys, ctc_weight=W)[1] is None
    assert confidence.confidence_batch(model.avsr, xs, ys, ctc_weight=0.0)[1] is None


def test_bf16_engine(utts):
    m = _model(torch.bfloat16)
    x, y = utts[0][3], utts[1][3]
    c, = confidence.confidence_batch(m.avsr, [x], [y], ctc_weight=W, alternatives=K)
    lg = _device_scores(m.avsr, [x], [y])[0][0]
    ref = R.neighbors(torch.log_softmax(lg.double(), -1), y, int(x.shape[0]), m.avsr.blank, m.avsr.eos)
    want = R.posteriors(ref[0], ref[1], y, blank=m.avsr.blank, eos=m.avsr.eos)
    bound = _ctc_bound(ref, 1e-3)
    err = max(abs(t.ctc - p) for t, (p, _) in zip(c.tokens, want))
    print(f"bf16: max |d conf_ctc| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert all(0.0 < t.joint <= 1.0 and 0.0 < t.decoder <= 1.0 for t in c.tokens)


def test_words_zip_with_word_times(model, utts, conf):
    x, y, c = utts[0][3], utts[1][3], conf[3]
    ali, = align.align_batch(model.avsr, [x], [y])
    times = align.word_times(ali.spans, TOKENS, frame_rate=25.0)
    for agg in ("min", "prod", "mean"):
        words = confidence.word_confidences(c.tokens, TOKENS, agg=agg)
        assert [w for w, _ in words] == [w for w, _, _ in times]
        assert all(0.0 < v <= 1.0 for _, v in words)

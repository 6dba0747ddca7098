"""avsr_amd.kws on the tiny model (oracle.weights.TINY_CONFIG, golden weights, eval, fp32 engine):
the property that ties keyword spotting to greedy CTC decoding, batch independence, the
CTCHead.spot_keywords call form, and occurrences."""
import pytest
import torch

from avsr_amd import kws
from avsr_amd.avhubert_avsr_model import AVHubertAVSR
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests.oracle_util import golden_state, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(dev):
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT)).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(load_golden()).items()}, strict=True)
    m.setup_engine("cuda", torch.float32)
    return m


@pytest.fixture(scope="module")
def utts(model):
    """encoded utterances of 25 and 19 frames, and per utterance the frame argmax of the CTC head"""
    g = load_golden()
    xs = [torch.from_numpy(g[f"dec_enc_{b}"]).cuda() for b in range(2)]
    assert [int(x.shape[0]) for x in xs] == [25, 19]
    am = [model.avsr.ctc.argmax(x.unsqueeze(0))[0].tolist() for x in xs]
    return xs, am


def _collapse(frames, blank=0):
    """greedy CTC reading of a run of frames: merge repeats, drop blanks"""
    out, prev = [], blank
    for a in frames:
        if a != prev and a != blank:
            out.append(a)
        prev = a
    return out


def _substrings(g, eos):
    """every contiguous g[i:j] of 1 to 4 tokens, once each, in order of first appearance (eos is
    no CTC label: check_keywords refuses it, so a substring holding it is left out)"""
    seen = []
    for i in range(len(g)):
        for j in range(i + 1, min(i + 4, len(g)) + 1):
            y = g[i:j]
            if eos not in y and y not in seen:
                seen.append(y)
    return seen


def hits_of(hits, keyword):
    return next(h for h in hits if h.keyword == keyword)


@pytest.fixture(scope="module")
def spotted(model, utts):
    """per utterance (keywords = the substrings of its greedy reading, their hits alone)"""
    xs, am = utts
    out = []
    for x, a in zip(xs, am):
        kw = _substrings(_collapse(a), model.avsr.eos)
        assert len(kw) >= 4
        out.append((kw, kws.spot_batch(model.avsr, [x], kw)[0]))
    return out


def test_greedy_substrings_score_zero(model, utts, spotted):
    """a keyword that the greedy reading contains is found with score exactly 0.0 (every frame of
    its span is the frame's best token), over a span whose greedy reading is the keyword; a
    keyword with a token that is no frame's argmax scores below 0"""
    xs, am = utts
    e2e = model.avsr
    for u, (kw, hits) in enumerate(spotted):
        assert sorted(h.keyword for h in hits) == list(range(len(kw)))           # T >= 4 + repeats: all fit
        assert hits == sorted(hits, key=lambda h: (h.start, h.end, h.keyword))
        for h in hits:
            assert h.score == 0.0 and h.avg == 0.0, (u, kw[h.keyword], h)
            assert 0 <= h.start < h.end <= len(am[u])
            assert _collapse(am[u][h.start:h.end]) == kw[h.keyword], (u, kw[h.keyword], h)
        absent = next(t for t in range(1, e2e.eos) if t not in am[u])
        said = kw[0][0]
        other = kws.spot_batch(e2e, [xs[u]], [[absent], [said, absent], [absent, said]])[0]
        assert len(other) == 3 and all(h.score < 0.0 and h.avg < 0.0 for h in other)
        assert kws.spot_batch(e2e, [xs[u]], [[absent], kw[0]], threshold=0.0)[0] == [hits_of(hits, 0)._replace(keyword=1)]


def test_batch_independent(model, utts, spotted):
    """an utterance's hits are identical alone and in a batch of two"""
    xs, _ = utts
    for u, (kw, alone) in enumerate(spotted):
        both = kws.spot_batch(model.avsr, xs, kw)
        assert len(both) == 2 and both[u] == alone
        assert kws.spot_batch(model.avsr, xs[::-1], kw)[1 - u] == alone
    assert kws.spot_batch(model.avsr, [], [[1]]) == []


def test_call_form(model, utts, spotted):
    """CTCHead.spot_keywords(h, keywords) is spot_batch on that utterance; (T, D) or (1, T, D),
    host or device input; bad keywords are refused before anything runs"""
    xs, _ = utts
    ctc = model.avsr.ctc
    for x, (kw, alone) in zip(xs, spotted):
        assert ctc.spot_keywords(x, kw) == alone
    kw, alone = spotted[1]
    assert ctc.spot_keywords(xs[1].unsqueeze(0).cpu(), kw) == alone
    assert ctc.spot_keywords(xs[1], kw, threshold=0.0) == alone      # avg = 0.0 passes a threshold of 0
    with pytest.raises(ValueError):
        ctc.spot_keywords(xs[0], [[0]])
    with pytest.raises(ValueError):
        ctc.spot_keywords(xs[0], [])
    with pytest.raises(ValueError):
        ctc.spot_keywords(xs[0].unsqueeze(0).expand(2, -1, -1), [[1]])


def test_occurrences(model, utts, spotted):
    """occurrences=True: per keyword non-overlapping spans sorted by start, the best hit among them"""
    xs, _ = utts
    for u, (kw, best) in enumerate(spotted):
        occ = kws.spot_batch(model.avsr, [xs[u]], kw, occurrences=True)[0]
        assert occ == sorted(occ, key=lambda h: (h.start, h.end, h.keyword))
        for b in best:
            mine = [h for h in occ if h.keyword == b.keyword]
            assert b in mine
            assert all(x.end <= y.start for x, y in zip(mine, mine[1:]))
            assert all(h.score <= b.score for h in mine)
        near = kws.spot_batch(model.avsr, [xs[u]], kw, threshold=-0.5, occurrences=True)[0]
        assert all(h.avg >= -0.5 for h in near) and all(b in near for b in best)

"""Two-pass decoding (avsr_amd/rescore.py) on the tiny model (oracle.weights.TINY_CONFIG, gen_tensor
weights at seed 0, fp32, eval: the model of tests/golden/make_golden_ctcw.py).

The second pass is checked against the REFERENCE: every hypothesis the reference's search returned
in tests/golden/avsr_ctcw.npz, stripped of sos / eos and rescored, must get the reference's own
`decoder` score (w = 0 entries) and `ctc` score (w = 1 entries) within the project's rule
1e-4 * |s| + 1e-4 (tests/decode_ref.py uses it for the same quantities).

What the goldens hold, which fixes how they are compared: the random tiny model never ends a
hypothesis by itself, so every golden hypothesis ran to maxlen = T and got its final eos APPENDED
WITHOUT A SCORE (batch_beam_search.py:320-330). Hence
  * the reference's `decoder` score of [sos] + y + [eos] is the sum over the L targets y alone;
    it is compared with the first L of the L + 1 per-target log-probs the second pass returns
    (Hypothesis.states["decoder"]), and the remaining eos term with the CPU oracle's
    decoder_one_step (pinned to the reference in tests/test_oracle_golden.py) under the same rule;
  * some w = 1 hypotheses CHOSE eos at the last step and then got the appended one as well
    ([.., eos, eos]): every trailing eos is stripped; their `ctc` score is the full-sequence
    probability of the remaining tokens. The others have L = T tokens without adjacent repeats,
    where the prefix probability the reference accumulated equals the full-sequence probability
    (one frame per token).

The first pass is checked on the same model with its CTC head sharpened (ctc_lo x 40: the random
head's posteriors are flat, maximum probability 6e-4, and every case would skip): the engine's own
log-softmax bits go to the fp64 restatement tests/ctc_beam_ref.py."""
import os

import numpy as np
import pytest
import torch

from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_rescoring_decoder
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from avsr_amd.rescore import ctc_feasible
from oracle import avsr_oracle as O
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests import ctc_beam_ref as R
from tests.oracle_util import golden_state, load_golden, tiny_cfg

pytestmark = pytest.mark.gpu

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
EOS = 5048
# bf16 engine: the largest relative deviation of the second pass from the reference's scores over
# the avsr_ctcw hypotheses, as measured on an MI355X; asserted at twice that
BF16_DEC_DEV = 1.701e-4
BF16_CTC_DEV = 1.594e-4


def close(got, ref):
    return abs(got - ref) <= 1e-4 * abs(ref) + 1e-4


@pytest.fixture(scope="module")
def g():
    return load_golden()


def _model(g, dtype, sharpen=1.0):
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT)).eval()
    sd = {k: torch.from_numpy(v) for k, v in golden_state(g).items()}
    for k in ("avsr.ctc.ctc_lo.weight", "avsr.ctc.ctc_lo.bias"):
        sd[k] = sd[k] * sharpen
    m.load_state_dict(sd, strict=True)
    m.setup_engine("cuda", dtype)
    return m


@pytest.fixture(scope="module")
def model(g, dev):
    return _model(g, torch.float32)


@pytest.fixture(scope="module")
def sharp(g, dev):
    return _model(g, torch.float32, sharpen=40.0)


@pytest.fixture(scope="module")
def xs(g):
    return [torch.from_numpy(g[f"dec_enc_{b}"]).cuda() for b in range(2)]


def strip(yseq):
    y = list(yseq[1:])
    while y and y[-1] == EOS:
        y.pop()
    return y


@pytest.fixture(scope="module")
def golden():
    """per clip and scorer: [(label sequence, the reference's score of that scorer)]"""
    c = np.load(os.path.join(os.path.dirname(__file__), "golden", "avsr_ctcw.npz"))
    out = {}
    for w, scorer in ((0, "decoder"), (1, "ctc")):
        for b in range(2):
            rows = []
            for beam in (1, 3):
                key = f"w{w}_b{beam}_{b}"
                ys = np.split(c[key + "_yseq"], np.cumsum(c[key + "_len"])[:-1])
                rows += [(strip(y.tolist()), float(s)) for y, s in zip(ys, c[key + "_" + scorer])]
            out[scorer, b] = rows
    assert all(len(v) == 4 for v in out.values())
    return out


def by_seq(hyps):
    return {tuple(h.yseq.tolist()[1:-1]): h for h in hyps}


def dec_dev(search, x, rows):
    """relative deviations of the first-L decoder sums from the reference's decoder scores"""
    got = by_seq(search.rescore(x, [y for y, _ in rows]))
    return [(float(got[tuple(y)].states["decoder"][:len(y)].double().sum()), s) for y, s in rows]


def test_decoder_scores_match_reference(g, model, xs, golden):
    search = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=0.0)
    sd, cfg = O.to_torch_state(golden_state(g)), tiny_cfg()
    for b in range(2):
        rows = golden["decoder", b]
        hyps = search.rescore(xs[b], [y for y, _ in rows])
        assert all(set(h.scores) == {"decoder"} for h in hyps)
        assert [float(h.score) for h in hyps] == sorted((float(h.score) for h in hyps), reverse=True)
        got = by_seq(hyps)
        for y, ref in rows:
            h = got[tuple(y)]
            tok = h.states["decoder"].double()
            assert h.yseq.tolist() == [EOS] + y + [EOS] and tok.numel() == len(y) + 1
            first = float(tok[:len(y)].sum())
            print(f"clip {b} L {len(y)} decoder {first:.6f} ref {ref:.6f}")
            assert close(first, ref)
            with torch.no_grad():
                eos_ref = float(O.decoder_one_step(sd, cfg, torch.tensor([[EOS] + y]), xs[b].cpu().unsqueeze(0))[0, EOS])
            print(f"   eos term {float(tok[-1]):.6f} oracle {eos_ref:.6f}")
            assert close(float(tok[-1]), eos_ref)
            assert float(h.scores["decoder"]) == float(tok.sum()) == float(h.score)


def test_ctc_scores_match_reference(model, xs, golden):
    search = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=1.0)
    for b in range(2):
        rows = golden["ctc", b]
        hyps = search.rescore(xs[b], [y for y, _ in rows])
        assert all(set(h.scores) == {"ctc"} and h.states == {} for h in hyps)
        got = by_seq(hyps)
        for y, ref in rows:
            h = got[tuple(y)]
            print(f"clip {b} L {len(y)} ctc {float(h.scores['ctc']):.6f} ref {ref:.6f}")
            assert close(float(h.scores["ctc"]), ref)
            assert float(h.score) == float(h.scores["ctc"])


@pytest.mark.parametrize("w", [0.1, 0.5])
def test_joint_score_identity(model, xs, golden, w):
    """score = (1 - w) * decoder + w * ctc on every golden hypothesis of a clip in one call; the
    w = 0 hypotheses have L = T tokens WITH adjacent repeats, so they are infeasible for CTC:
    ctc = score = -inf, sorted last"""
    search = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=w)
    for b in range(2):
        ys = [y for y, _ in golden["decoder", b] + golden["ctc", b]]
        hyps = search.rescore(xs[b], ys)
        assert len(hyps) == len(ys) and all(set(h.scores) == {"decoder", "ctc"} for h in hyps)
        scores = [float(h.score) for h in hyps]
        assert scores == sorted(scores, reverse=True)
        got = by_seq(hyps)
        for y, ref in golden["ctc", b]:
            h = got[tuple(y)]
            assert close(float(h.scores["ctc"]), ref)
            assert float(h.score) == (1 - w) * float(h.scores["decoder"]) + w * float(h.scores["ctc"])
        for y, ref in golden["decoder", b]:
            h = got[tuple(y)]
            assert close(float(h.states["decoder"][:len(y)].double().sum()), ref)
            assert not ctc_feasible(xs[b].shape[0], y)
            assert float(h.scores["ctc"]) == float(h.score) == float("-inf")
        assert all(s == float("-inf") for s in scores[-4:]) and all(s > float("-inf") for s in scores[:-4])


def test_empty_hypothesis(model, xs):
    logp = model.avsr.ctc.log_softmax(xs[0].unsqueeze(0))[0]
    blank_sum = float(logp[:, 0].double().sum())
    h = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=1.0).rescore(xs[0], [[]])[0]
    assert h.yseq.tolist() == [EOS, EOS]
    assert close(float(h.scores["ctc"]), blank_sum)
    both = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=0.5).rescore(xs[0], [[], [5, 17]])
    e = by_seq(both)[()]
    assert close(float(e.scores["ctc"]), blank_sum) and e.states["decoder"].numel() == 1


def test_infeasible_hypothesis_sorts_last(model, xs):
    """8 frames, 6 equal tokens need 11: avsr_ctc_fwd's zero_infinity would report nll 0"""
    for w in (1.0, 0.3):
        hyps = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=w).rescore(xs[0][:8], [[7] * 6, [7, 8, 9]])
        assert [h.yseq.tolist()[1:-1] for h in hyps] == [[7, 8, 9], [7] * 6]
        assert float(hyps[1].scores["ctc"]) == float("-inf") == float(hyps[1].score)
        assert np.isfinite(float(hyps[0].score))


def test_mixed_lengths_score_as_alone(model, xs):
    """hypotheses of different lengths in one call (padded with eos, target -1) against one call
    each; the GEMM row count differs between the two, so the project's rule, not equality"""
    search = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=0.5)
    ys = [[], [5, 17, 301], [9, 8, 7, 6, 5, 4, 3, 2, 11]]
    together = by_seq(search.rescore(xs[1], ys))
    for y in ys:
        alone = search.rescore(xs[1], [y])[0]
        t = together[tuple(y)]
        assert t.states["decoder"].numel() == len(y) + 1
        for k in ("decoder", "ctc"):
            assert close(float(t.scores[k]), float(alone.scores[k])), (y, k)


@pytest.mark.parametrize("N,C", [(4, 8), (10, 16)])
def test_first_pass_matches_restatement(sharp, xs, N, C):
    search = get_rescoring_decoder(sharp.avsr, TOKENS, beam_size=N, token_beam=C)
    got = search.ctc_nbest(xs)
    for b in range(2):
        logp = sharp.avsr.ctc.log_softmax(xs[b].unsqueeze(0))[0].cpu().numpy()
        T = logp.shape[0]
        ref = R.search(logp, R.topk_ids(logp, C), N, blank=0, eos=EOS, Lcap=T)
        print(f"clip {b} (N, C) = ({N}, {C}) margin {ref['margin']:.2f}")
        assert ref["margin"] >= 1                                   # these clips must not skip
        assert [tuple(y) for y, _ in got[b]] == [h for h, _ in ref["hyps"]]
        for (_, s), (_, r) in zip(got[b], ref["hyps"]):
            assert abs(s - r) <= R.tol(r, T), (s, r)


def same(a, b):
    return ([h.yseq.tolist() for h in a] == [h.yseq.tolist() for h in b]
            and [float(h.score) for h in a] == [float(h.score) for h in b]
            and [{k: float(v) for k, v in h.scores.items()} for h in a] == [{k: float(v) for k, v in h.scores.items()} for h in b])


def test_composition(sharp, xs):
    search = get_rescoring_decoder(sharp.avsr, TOKENS, ctc_weight=0.3, beam_size=4, token_beam=8)
    alone = [search(x) for x in xs]
    for x, a in zip(xs, alone):
        assert 1 <= len(a) <= 4 and a[0].yseq[0] == EOS and a[0].yseq[-1] == EOS
        assert same(a, search.rescore(x, search.ctc_nbest([x])[0]))
    assert all(same(a, d) for a, d in zip(alone, search.decode_batch(xs)))
    assert all(same(a, d) for a, d in zip(alone[::-1], search.decode_batch(xs[::-1])))


def test_bf16_engine_against_reference(g, xs, golden, dev):
    """the yardstick is the reference's golden, never the fp32 engine. One bf16 rounding of a
    logit moves a log-prob by up to 2^-9 relative; how that accumulates through this decoder is
    not derivable here, so the bound is twice the largest deviation measured on an MI355X (the
    factor 2 covers box-to-box GEMM tile differences)."""
    m = _model(g, torch.bfloat16)
    dec = get_rescoring_decoder(m.avsr, TOKENS, ctc_weight=0.0)
    ctc = get_rescoring_decoder(m.avsr, TOKENS, ctc_weight=1.0)
    worst_d = worst_c = 0.0
    for b in range(2):
        for got, ref in dec_dev(dec, xs[b], golden["decoder", b]):
            worst_d = max(worst_d, abs(got - ref) / abs(ref))
        rows = golden["ctc", b]
        hyps = by_seq(ctc.rescore(xs[b], [y for y, _ in rows]))
        for y, ref in rows:
            worst_c = max(worst_c, abs(float(hyps[tuple(y)].scores["ctc"]) - ref) / abs(ref))
    print(f"bf16 largest relative deviation: decoder {worst_d:.3e} ctc {worst_c:.3e}")
    assert worst_d <= 2 * BF16_DEC_DEV and worst_c <= 2 * BF16_CTC_DEV

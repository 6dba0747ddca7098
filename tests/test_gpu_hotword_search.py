"""The beam search with hot-word biasing: the real step sequence (BatchBeamSearch._step /
_capture / _collect, unchanged) on a table decoder against the fp64 restatement in
tests/hotword_ref.py, eager and as two replayed graphs, batched and one utterance at a time; the
search without a phrase list; and the real (tiny) model through the public interface.
The cases and what they cover are fixed in hotword_ref.SEARCH_CASES and checked without a GPU by
tests/test_hotword_host.py."""
import types

import pytest
import torch

from avsr_amd import hotwords as HW
from avsr_amd import ops
from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder, get_rescoring_decoder
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from avsr_amd.decode import BatchBeamSearch
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests import hotword_ref as H
from tests.oracle_util import golden_state, load_golden

pytestmark = pytest.mark.gpu


class ScriptedSearch(BatchBeamSearch):
    """BatchBeamSearch whose decoder is a table: row r at position i with last token t gets the
    logits table[u][i][t][:], through the real log-softmax + pre-beam kernel (the pattern of
    tests/test_gpu_decode_scripted.py)"""

    def __init__(self, table, beam, w):
        V = table.shape[-1]
        super().__init__(None, beam_size=beam, vocab_size=V, weights={"decoder": 1.0 - w, "ctc": w}, sos=V - 1,
                         eos=V - 1, pre_beam_score_key=None if w == 1.0 else "decoder")
        self.table = table

    def _decoder_step(self, eng, st):
        R_, V = st["R"], self.n_vocab
        logits = self.table[st["uidx"].long(), st["pos"].long().expand(R_), st["tok"].long()].contiguous()
        logp = torch.empty(R_, V, device=logits.device, dtype=torch.float32)
        return ops.log_softmax_topk(logits, V, logp, self.pre_beam_size, st["ids"])

    def run(self, ctc_logp, Ts, graphs=False):
        """decode_batch without an engine: the state, step 0 eagerly, then eager steps or, as
        decode_batch does, replays of the two captured graphs, until every utterance is done"""
        U = len(Ts)
        st = self.state = self._new_state(ctc_logp.device, torch.float32, Ts, Ts, ctc_logp, None, 64, 0, end_detect=1)
        self._step(None, st, True, 0)
        replay = None
        if graphs and st["steps"] > 1:
            eng = types.SimpleNamespace(device=ctc_logp.device, dH=1)      # what _capture reads of an engine
            replay = self._capture(eng, st)
        for i in range(1, st["steps"]):
            if int(st["done"][U].item()) == U:
                break
            if replay is not None:
                replay[i & 1].replay()
            else:
                self._step(None, st, False, i & 1)
        torch.cuda.synchronize()
        return [[h.asdict() for h in nbest] for nbest in self._collect(st, [None] * U, 0.0, 0.0)]


def _search(dev, c, rows=None, graphs=False, hotwords=True):
    """the batched search of case inputs c, or of utterance `rows` alone (its own buffers, Tm = T_u)"""
    if rows is None:
        table, ctc, Ts = c["table"], c["ctc"], c["Ts"]
    else:
        T = c["Ts"][rows]
        table, ctc, Ts = c["table"][rows:rows + 1, :T], c["ctc"][rows:rows + 1, :T], [T]
    bs = ScriptedSearch(table.to(dev).contiguous(), c["beam"], c["w"])
    if hotwords is True:
        bs.set_hotwords(c["phrases"], c["beta"])
    elif hotwords is not False:
        bs.set_hotwords(c["phrases"], c["beta"])
        bs.set_hotwords(hotwords)                    # None or []: cleared again
    return bs.run(ctc.to(dev).contiguous(), Ts, graphs), bs


def _assert_matches_reference(got, want):
    """n-best token sequences equal in order; total and per-scorer scores, hotword included,
    within 1e-4 relative"""
    assert [h["yseq"] for h in got] == [h.yseq for h in want]
    for h, r in zip(got, want):
        assert abs(h["score"] - r.score) <= 1e-4 * abs(r.score), (h["score"], r.score)
        assert set(h["scores"]) == set(r.scores) == {"decoder", "ctc", "hotword"}
        for k in r.scores:
            assert abs(h["scores"][k] - r.scores[k]) <= 1e-4 * abs(r.scores[k]), (k, h["scores"][k], r.scores[k])


@pytest.mark.parametrize("case", H.SEARCH_CASES, ids=lambda c: f"s{c[0]}-b{c[1]}-w{c[2]:g}-{c[3]}-beta{c[4]:g}")
def test_hotword_search_matches_fp64_reference(dev, case):
    """every case (none is skipped): the n-best lists of the device search equal the reference's;
    the batched result equals the one-utterance search with ==, floats included; and the two-graph
    replay equals the eager step sequence with =="""
    c, refs = H.search_reference(case)
    got, bs = _search(dev, c)
    st = bs.state
    Pw = bs.pre_beam_size + H.C
    assert st["ids"].shape[1] == bs.pre_beam_size and st["hw"]["ids"].shape[1] == Pw
    assert st["psi"].shape[1] == Pw + 1 and st["r_new"].shape[1] == Pw
    replayed, _ = _search(dev, c, graphs=True)
    assert replayed == got
    for u, (want, *_) in enumerate(refs):
        alone, _ = _search(dev, c, rows=u)
        assert got[u] == alone[0], u
        _assert_matches_reference(got[u], want)


@pytest.mark.parametrize("clear", [None, []], ids=["none", "empty"])
@pytest.mark.parametrize("case", H.CLEARED_CASES, ids=lambda c: f"s{c[0]}-b{c[1]}")
def test_cleared_list_is_the_plain_search(dev, case, clear):
    """set_hotwords(None) / an empty list after a list was set: results == the search that never had
    one, eager and replayed; the state holds no hot-word buffer and the candidate arrays keep their P
    columns; and that search is the fp64 reference without phrases"""
    c, refs = H.search_reference(case)
    plain, bs0 = _search(dev, c, hotwords=False)
    for graphs in (False, True):
        got, bs = _search(dev, c, graphs=graphs, hotwords=clear)
        assert got == plain
        st, P = bs.state, bs.pre_beam_size
        assert bs.hotwords is None and "hw" not in st and "bonus" not in st["out"] and "next" not in st["out"]
        assert st["ids"].shape[1] == P and st["psi"].shape[1] == P + 1 and st["r_new"].shape[1] == P
        assert sorted(st) == sorted(bs0.state)
    for u, (_, _, want, *_) in enumerate(refs):
        assert [h["yseq"] for h in plain[u]] == [h.yseq for h in want]
        assert all(set(h["scores"]) == {"decoder", "ctc"} for h in plain[u])


# ------------------------------------------------------------------------------ the real model
TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
EOS = len(TOKENS) - 1


@pytest.fixture(scope="module")
def g():
    return load_golden()


@pytest.fixture(scope="module")
def model(g):
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT)).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    m.setup_engine("cuda", torch.float32)
    return m


def _pairs(yseq):
    body = [t for t in yseq[1:] if t != EOS]
    return list(zip(body, body[1:]))


def _walk_sum(tree, yseq, T):
    """the k of a hypothesis's own tokens: sos is not walked, nor the eos a length limit appends
    (maxlen = T: such a hypothesis has sos + T tokens + eos)"""
    toks = yseq[1:-1] if len(yseq) == T + 2 else yseq[1:]
    return sum(tree.walk(toks)[0])


def test_model_top_hypothesis_takes_the_span(g, model):
    """beam 3 on the reference's encoder output: a 2-token span of the plain search's second
    hypothesis that its best lacks, as the only phrase at beta = 5, is in the new top hypothesis;
    its score is the documented sum of its parts and its hot-word score the walk of its own tokens"""
    x = torch.from_numpy(g["dec_enc_0"]).cuda()
    T = x.shape[0]
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    plain = [h.asdict() for h in bs(x)]
    assert len(plain) >= 2
    have = set(_pairs(plain[0]["yseq"]))
    span = next(p for p in _pairs(plain[1]["yseq"]) if p not in have and 0 not in p)
    beta = 5.0
    bs.set_hotwords([list(span)], beta)
    top = bs(x)[0].asdict()
    print("span", span, "plain best", plain[0]["yseq"], "second", plain[1]["yseq"], "biased top", top["yseq"], top["scores"])
    assert span in _pairs(top["yseq"])
    sc = top["scores"]
    assert set(sc) == {"decoder", "ctc", "hotword"}
    total = 0.9 * sc["decoder"] + 0.1 * sc["ctc"] + sc["hotword"]
    assert abs(top["score"] - total) <= 1e-4 * abs(total), (top["score"], total)
    assert sc["hotword"] == beta * _walk_sum(HW.build_tree([list(span)], eos=EOS), top["yseq"], T)
    assert sc["hotword"] >= 2 * beta
    bs.set_hotwords(None)
    assert [h.asdict() for h in bs(x)] == plain


def test_model_batched_equals_alone(g, model):
    """decode_batch of 3 utterances of different lengths with a phrase list == each alone"""
    xs = [torch.from_numpy(g["dec_enc_0"]).cuda(), torch.from_numpy(g["dec_enc_1"]).cuda(),
          torch.from_numpy(g["dec_enc_0"][:11]).cuda()]
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    first = [[h.asdict()["yseq"] for h in nbest] for nbest in bs.decode_batch(xs)]      # per utterance, best first
    phrases = [y[0][1:3] for y in first if len(y[0]) >= 4 and EOS not in y[0][1:3] and 0 not in y[0][1:3]]
    phrases += [y[-1][2:5] for y in first if len(y[-1]) >= 6 and EOS not in y[-1][2:5] and 0 not in y[-1][2:5]]
    assert phrases
    bs = get_beam_search_decoder(model.avsr, TOKENS, 0.1, 3, phrases, 2.0)
    got = bs.decode_batch(xs)
    assert any(h.asdict()["scores"]["hotword"] != 0.0 for nbest in got for h in nbest)
    for x, hyps in zip(xs, got):
        assert [h.asdict() for h in hyps] == [h.asdict() for h in bs(x)]


def test_model_refused_modes_only_with_a_list(g, model):
    x = torch.from_numpy(g["dec_enc_0"][:11]).cuda()
    phrases = [[5, 6]]
    for w in (0.0, 1.0):
        bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=w, beam_size=3)
        bs.set_hotwords(None)
        assert bs(x)                                             # as before without a list
        with pytest.raises(NotImplementedError):
            bs.set_hotwords(phrases, 1.0)
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    want = [h.asdict() for h in bs(x)]
    assert [h.asdict() for h in bs.decode_stream([x], slots=1, max_frames=16)[0]] == want
    bs.set_hotwords(phrases, 1.0)
    with pytest.raises(NotImplementedError):
        bs.stream(slots=1, max_frames=16)
    with pytest.raises(NotImplementedError):
        bs.decode_stream([x], slots=1, max_frames=16)
    bs.set_hotwords([])
    assert [h.asdict() for h in bs.decode_stream([x], slots=1, max_frames=16)[0]] == want
    two = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    two.set_hotwords(None)
    assert two(x)
    with pytest.raises(NotImplementedError):
        two.set_hotwords(phrases, 1.0)
    with pytest.raises(NotImplementedError):
        get_rescoring_decoder(model.avsr, TOKENS, hotwords=phrases, hotword_bonus=1.0)

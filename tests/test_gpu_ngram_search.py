"""The beam search with n-gram LM shallow fusion and the length bonus: the real step sequence
(BatchBeamSearch._step / _capture / _collect) on a table decoder against the fp64 restatement in
tests/ngram_ref.py, eager and as two replayed graphs, batched and one utterance at a time, with and
without a hot-word list; the search after set_lm(None, 0.0); the refused forms; and the two-pass
decoder on the real (tiny) model. The cases and what they cover are fixed in ngram_ref.SEARCH_CASES
and checked without a GPU by tests/test_ngram_host.py."""
import numpy as np
import pytest
import torch

from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder, get_rescoring_decoder
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from avsr_amd.ngram_lm import NgramLM
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests import ngram_ref as N
from tests.oracle_util import golden_state, load_golden
from tests.test_gpu_hotword_search import ScriptedSearch

pytestmark = pytest.mark.gpu


def _lm(order):
    ent = {k: v for k, v in N.SEARCH_TABLE.items() if len(k[0]) + 1 <= order}
    return NgramLM.from_table(order, ent, N.SOS, N.EOS, N.V, N.UNK)


def _search(dev, c, rows=None, graphs=False, fused=True):
    """the batched search of case inputs c, or of utterance `rows` alone (its own buffers, Tm = T_u).
    fused False: never had an LM; "cleared": had one, then set_lm(None, 0.0)"""
    if rows is None:
        table, ctc, Ts = c["table"], c["ctc"], c["Ts"]
    else:
        T = c["Ts"][rows]
        table, ctc, Ts = c["table"][rows:rows + 1, :T], c["ctc"][rows:rows + 1, :T], [T]
    bs = ScriptedSearch(table.to(dev).contiguous(), c["beam"], c["w"])
    if fused:
        bs.set_lm(None if c["order"] is None else _lm(c["order"]), c["w_lm"], c["w_len"])
        if c["phrases"] is not None and fused is True:
            bs.set_hotwords(c["phrases"], c["beta"])
    if fused == "cleared":
        bs.set_lm(None, 0.0)
    return bs.run(ctc.to(dev).contiguous(), Ts, graphs), bs


@pytest.mark.parametrize("case", N.SEARCH_CASES, ids=N.case_id)
def test_lm_search_matches_fp64_reference(dev, case):
    """every case (none is skipped): the n-best token sequences equal the reference's in order, total
    and per-scorer scores within 1e-4 relative; the two-graph replay == the eager step sequence; the
    batched result == the one-utterance search, floats included"""
    c, refs = N.search_reference(case)
    got, bs = _search(dev, c)
    st = bs.state
    assert ("arrays" in st["lm"]) == (c["order"] is not None) and ("slen" in st["lm"]) == (c["w_len"] != 0.0)
    if c["order"] is not None:
        assert st["lm"]["score"].shape[1] == st["psi"].shape[1]         # the widened columns are scored too
    replayed, _ = _search(dev, c, graphs=True)
    assert replayed == got
    for u, (want, *_) in enumerate(refs):
        alone, _ = _search(dev, c, rows=u)
        assert got[u] == alone[0], u
        assert [h["yseq"] for h in got[u]] == [h.yseq for h in want]
        for h, r in zip(got[u], want):
            assert abs(h["score"] - r.score) <= 1e-4 * abs(r.score), (h["score"], r.score)
            assert set(h["scores"]) == set(r.scores)
            for k in r.scores:
                assert abs(h["scores"][k] - r.scores[k]) <= 1e-4 * abs(r.scores[k]), (k, h["scores"][k], r.scores[k])


@pytest.mark.parametrize("case", [N.SEARCH_CASES[1], N.SEARCH_CASES[4]], ids=N.case_id)
def test_cleared_lm_is_the_plain_search(dev, case):
    """set_lm(None, 0.0) after an LM and a length bonus were set: results == the search that never
    had them, eager and replayed; the state holds no LM buffer; and that search is the fp64 reference
    without LM"""
    c, refs = N.search_reference(case)
    plain, bs0 = _search(dev, c, fused=False)
    for graphs in (False, True):
        got, bs = _search(dev, c, graphs=graphs, fused="cleared")
        assert got == plain
        st = bs.state
        assert bs.lm is None and "lm" not in st and "lm" not in st["out"] and "lm_next" not in st["out"]
        assert sorted(st) == sorted(bs0.state) and sorted(st["out"]) == sorted(bs0.state["out"])
        assert bs.weights["lm"] == 0.0 and bs.weights["length_bonus"] == 0.0
    for u, (_, _, want, _) in enumerate(refs):
        assert [h["yseq"] for h in plain[u]] == [h.yseq for h in want]
        assert all(set(h["scores"]) == {"decoder", "ctc"} for h in plain[u])


def test_refused_forms(dev):
    c, _ = N.search_reference(N.SEARCH_CASES[1])
    lm = _lm(2)
    for w in (0.0, 1.0):
        bs = ScriptedSearch(c["table"].to(dev), 3, w)
        bs.set_lm(None, 0.0)
        with pytest.raises(NotImplementedError, match="two-pass"):
            bs.set_lm(lm, 0.5)
        with pytest.raises(NotImplementedError):
            bs.set_lm(None, 0.0, 0.5)
    bs = ScriptedSearch(c["table"].to(dev), 3, 0.3)
    for kw in (dict(lm=lm, weight=0.5), dict(lm=None, weight=0.0, length_bonus=0.5)):
        bs.set_lm(**kw)
        with pytest.raises(NotImplementedError, match="decode_batch"):
            bs.stream(slots=1, max_frames=16)
        with pytest.raises(NotImplementedError, match="decode_batch"):
            bs.decode_stream([None], slots=1, max_frames=16)


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


def _d(h):
    """yseq, score and scores of a Hypothesis (states hold tensors)"""
    d = h.asdict()
    d.pop("states")
    return d


def _model_table(cands):
    """an order-3 table over the 5049-token vocabulary: unigrams of every token the candidates hold
    (the rest score unk_logp), and the bigrams / trigrams of every second candidate, so entries of
    each order are hit and others are backed off from"""
    rng = np.random.RandomState(7)
    ent = {((), EOS): (-2.5, -0.5)}
    for y in cands:
        for t in y:
            ent.setdefault(((), t), (N._q(rng.uniform(-4, -2)), N._q(rng.uniform(-1, -0.1))))
    for y in cands[::2]:
        h = [EOS] + list(y) + [EOS]
        for i in range(1, len(h)):
            ent.setdefault(((h[i - 1],), h[i]), (N._q(rng.uniform(-1.5, -0.5)), N._q(rng.uniform(-0.5, -0.1))))
            if i >= 2:
                ent.setdefault(((h[i - 2], h[i - 1]), h[i]), (N._q(rng.uniform(-0.5, -0.1)), 0.0))
    return ent


@pytest.mark.parametrize("w", [0.0, 0.1, 1.0])
def test_rescorer_with_lm_on_the_model(g, model, w):
    """the two-pass decoder at every kind of ctc_weight: with an LM and a length bonus the score,
    scores["lm"] and scores["length_bonus"] equal the fp64 recomputation from its own returned
    scores["decoder"] / scores["ctc"], the reference LM of the candidates and their lengths; the list
    is ranked by that score; rescore(x, yseqs) honours the LM too; the same candidates without an LM
    keep their scores =="""
    x = torch.from_numpy(g["dec_enc_0"]).cuda()
    plain_search = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=w, beam_size=10)
    plain = [_d(h) for h in plain_search(x)]
    cands = [h["yseq"][1:-1] for h in plain]
    assert len(cands) >= 3
    ent = _model_table(cands)
    lm = NgramLM.from_table(3, ent, EOS, EOS, len(TOKENS), -7.0)
    ref = N.RefLM(3, ent, -7.0, sos=EOS, eos=EOS)
    w_lm, w_len = 0.6, 0.4
    two = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=w, beam_size=10, lm=lm, lm_weight=w_lm, length_bonus=w_len)
    hyps = two(x)
    got = [_d(h) for h in hyps]
    assert sorted(h["yseq"] for h in got) == sorted(h["yseq"] for h in plain)        # the first pass is unchanged
    assert [h["score"] for h in got] == sorted((h["score"] for h in got), reverse=True)
    by_seq = {tuple(h["yseq"]): h for h in plain}
    want_keys = {"lm", "length_bonus"} | ({"decoder"} if w != 1.0 else set()) | ({"ctc"} if w != 0.0 else set())
    for h, d in zip(hyps, got):
        y = d["yseq"][1:-1]
        sc = d["scores"]
        assert set(sc) == want_keys
        p = by_seq[tuple(d["yseq"])]
        assert all(sc[k] == p["scores"][k] for k in p["scores"])                     # decoder / ctc: today's values
        lm_tok = ref.score_tokens(y)
        assert np.all(np.abs(h.states["lm"].numpy() - lm_tok) <= 1e-6 * np.abs(lm_tok))
        assert abs(sc["lm"] - sum(lm_tok)) <= 1e-6 * abs(sum(lm_tok)) and sc["length_bonus"] == len(y) + 1
        total = p["score"] + w_lm * sum(lm_tok) + w_len * (len(y) + 1)
        assert abs(d["score"] - total) <= 1e-6 * abs(total), (d["score"], total)
    assert [h["yseq"] for h in got] != [h["yseq"] for h in plain]                   # re-ranked
    again = [_d(h) for h in two.rescore(x, cands)]
    assert again == got
    two.set_lm(None, 0.0)
    assert [_d(h) for h in two(x)] == plain
    assert [_d(h) for h in plain_search.rescore(x, cands)] == plain


@pytest.mark.parametrize("setting", [0, 1])
def test_model_search_equals_the_reference_search(g, model, setting):
    """parity with the reference's own BatchBeamSearch given a LengthBonus and an n-gram scorer
    (tests/golden/avsr_lm.npz, tests/golden/make_golden_lm.py): through the public
    get_beam_search_decoder(..., lm=, lm_weight=, length_bonus=) on the tiny model the whole returned
    list equals the fixture's: tokens equal, total and per-scorer scores within 1e-4 relative"""
    fx = N.load_lm_fixture()
    w_lm, w_len = fx["settings"][setting]
    lm = NgramLM.from_table(fx["order"], fx["entries"], EOS, EOS, len(TOKENS), fx["unk"])
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3, lm=lm, lm_weight=w_lm, length_bonus=w_len)
    assert bs.weights == {"decoder": 0.9, "ctc": 0.1, "lm": w_lm, "length_bonus": w_len}
    xs = [torch.from_numpy(g[f"dec_enc_{c}"]).cuda() for c in range(2)]
    batched = bs.decode_batch(xs)
    for c, x in enumerate(xs):
        want = fx["runs"][(setting, c)]["hyps"]
        got = [_d(h) for h in bs(x)]
        assert got == [_d(h) for h in batched[c]]
        assert [h["yseq"] for h in got] == [h["yseq"] for h in want]
        for h, r in zip(got, want):
            assert abs(h["score"] - r["score"]) <= 1e-4 * abs(r["score"]), (h["score"], r["score"])
            assert set(h["scores"]) == set(r["scores"])
            for k, v in r["scores"].items():
                assert abs(h["scores"][k] - v) <= 1e-4 * abs(v), (k, h["scores"][k], v)
    bs.set_lm(None, 0.0)
    plain = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    assert [_d(h) for h in bs(xs[0])] == [_d(h) for h in plain(xs[0])]
    assert [int(t) for t in plain(xs[0])[0].yseq] == g["yseq_b3_0"].tolist()

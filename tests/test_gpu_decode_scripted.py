"""The real search step sequence (BatchBeamSearch._step / _collect, unchanged: beam_step_prep,
batched ctc_prefix with the device-side length, the full-vocabulary scoring of ctc_weight = 1,
beam_select over segments, beam_post, both gather_rows) with the neural decoder swapped for a
table of logits, against the fp64 restatement in tests/decode_ref.py. The cases, and which of them
are skipped because the reference's own top scores are closer than twice the tolerance, are fixed in
decode_ref.SCRIPTED_BATCHES and checked without a GPU by tests/test_decode_scripted_cases.py."""
import pytest
import torch

from avsr_amd import ops
from avsr_amd.decode import BatchBeamSearch
from tests import decode_ref as R

pytestmark = pytest.mark.gpu


class ScriptedSearch(BatchBeamSearch):
    """BatchBeamSearch whose decoder is a table: row r at position i with last token t gets the
    logits table[u][i][t][:], through the real log-softmax + pre-beam kernel"""

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

    def run(self, ctc_logp, Ts, maxlenratio=0.0):
        """decode_batch without an engine: the state, then the eager steps until every utterance is done"""
        U = len(Ts)
        maxlens = [T if maxlenratio == 0 else max(1, int(maxlenratio * T)) for T in Ts]
        st = self._new_state(ctc_logp.device, torch.float32, Ts, maxlens, ctc_logp, None, 64, 0,
                             end_detect=int(maxlenratio == 0.0))
        for i in range(st["steps"]):
            self._step(None, st, i == 0, i & 1)
            if int(st["done"][U].item()) == U:
                break
        return [[h.asdict() for h in nbest] for nbest in self._collect(st, [None] * U, maxlenratio, 0.0)]


def _search(dev, c, rows=None):
    """the batched search of case inputs c, or of utterance `rows` alone (its own buffers, Tm = T_u)"""
    if rows is None:
        table, ctc, Ts = c["table"], c["ctc"], c["Ts"]
    else:
        T = c["Ts"][rows]
        table, ctc, Ts = c["table"][rows:rows + 1, :T], c["ctc"][rows:rows + 1, :T], [T]
    bs = ScriptedSearch(table.to(dev).contiguous(), c["beam"], c["w"])
    return bs.run(ctc.to(dev).contiguous(), Ts, c["maxlenratio"])


def _assert_matches_reference(got, want, w):
    """n-best token sequences equal in order; total and per-scorer scores within 1e-4 relative"""
    assert [h["yseq"] for h in got] == [h.yseq for h in want]
    keys = {k for k, use in (("decoder", w != 1.0), ("ctc", w != 0.0)) if use}
    for h, r in zip(got, want):
        assert abs(h["score"] - r.score) <= 1e-4 * abs(r.score), (h["score"], r.score)
        assert set(h["scores"]) == set(r.scores) == keys
        for k in keys:
            assert abs(h["scores"][k] - r.scores[k]) <= 1e-4 * abs(r.scores[k]), (k, h["scores"][k], r.scores[k])


@pytest.mark.parametrize("batch", R.SCRIPTED_BATCHES, ids=lambda b: f"s{b[0]}-b{b[1]}-w{b[2]:g}-{b[3]}")
def test_scripted_search_matches_fp64_reference(dev, batch):
    """every unskipped case: the n-best lists of the device search equal the reference's; and for
    every case, skipped or not, the batched result equals the one-utterance search with =="""
    c, refs = R.scripted_reference(batch)
    got = _search(dev, c)
    for u, (want, info, skipped) in enumerate(refs):
        alone = _search(dev, c, rows=u)[0]
        assert got[u] == alone, u                    # tokens, total and per-scorer scores as floats
        if not skipped:
            _assert_matches_reference(got[u], want, c["w"])


def test_scripted_search_through_the_fallback_prefix_kernel(dev):
    """Tm = 250 at ctc_weight = 1 (chunks of P = 64 ids: 250 * 67 * 4 B of LDS would not fit, so
    the non-LDS prefix kernel scores the vocabulary), 12 steps (maxlenratio 0.05)"""
    c = R.long_case()
    assert 250 * (64 + 3) * 4 > 65536
    want, info = R.scripted_search_ref(c["table"][0], c["ctc"][0], c["beam"], c["w"], c["maxlenratio"])
    assert info["steps"] == 12 and info["margin"] >= 1.0
    got = _search(dev, c)[0]
    _assert_matches_reference(got, want, c["w"])

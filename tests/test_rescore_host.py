"""Host side of two-pass decoding (avsr_amd/rescore.py): argument validation, the CTC
feasibility rule, the fp64 score combination and ordering, and the search plugged into
evaluate.run_sharded through a stub. No GPU and no kernel call."""
import types

import numpy as np
import pytest
import torch

from avsr_amd import evaluate, rescore
from avsr_amd.avhubert_avsr_model import get_rescoring_decoder

V = 32
TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, V - 1)] + ["<eos>"]
STUB = types.SimpleNamespace(sos=V - 1, eos=V - 1, engine=lambda: types.SimpleNamespace(device="cpu"))


def test_defaults_and_validation():
    s = get_rescoring_decoder(STUB, TOKENS)
    assert (s.beam_size, s.token_beam, s.ctc_weight, s.sos, s.eos) == (10, 10, 0.1, V - 1, V - 1)
    assert get_rescoring_decoder(STUB, TOKENS, beam_size=16).token_beam == 16
    assert get_rescoring_decoder(STUB, TOKENS, beam_size=3, token_beam=16).token_beam == 16
    for kw in (dict(beam_size=0), dict(beam_size=17), dict(token_beam=0), dict(token_beam=17),
               dict(ctc_weight=-0.01), dict(ctc_weight=1.01)):
        with pytest.raises(ValueError):
            get_rescoring_decoder(STUB, TOKENS, **kw)
    both = get_rescoring_decoder(STUB, TOKENS, ctc_weight=0.5)
    assert both.use_dec and both.use_ctc
    dec_only, ctc_only = (get_rescoring_decoder(STUB, TOKENS, ctc_weight=w) for w in (0.0, 1.0))
    assert (dec_only.use_dec, dec_only.use_ctc, ctc_only.use_dec, ctc_only.use_ctc) == (True, False, False, True)


def test_feasibility_rule():
    """T >= L + adjacent repeats"""
    f = rescore.ctc_feasible
    assert f(0, []) and f(5, [])
    assert f(3, [1, 2, 3]) and not f(2, [1, 2, 3])
    assert not f(3, [1, 1, 2]) and f(4, [1, 1, 2])
    assert not f(8, [7] * 6) and not f(10, [7] * 6) and f(11, [7] * 6)
    assert f(3, [1, 2, 1])                        # equal but not adjacent


def test_joint_score_in_fp64():
    tok = np.array([-1.25, -0.5, -3.0000002], dtype=np.float32)
    ctc = np.float32(-7.123457)
    d64 = float(tok[0]) + float(tok[1]) + float(tok[2])
    s, d, c = rescore.joint_score(tok, ctc, 0.3)
    assert d == d64 and c == float(ctc) and s == 0.7 * d64 + 0.3 * float(ctc)
    assert rescore.joint_score(tok, None, 0.0) == (d64, d64, None)
    assert rescore.joint_score(None, ctc, 1.0) == (float(ctc), None, float(ctc))
    assert rescore.joint_score(tok, float("-inf"), 0.1)[0] == float("-inf")
    # a sum whose fp32 accumulation would lose the small terms
    many = np.array([-1000.0] + [-1e-5] * 1000, dtype=np.float32)
    assert rescore.joint_score(many, None, 0.0)[0] == float(np.sum(many.astype(np.float64)))


def _hyp(score, tag):
    return rescore.Hypothesis(yseq=torch.tensor([tag]), score=torch.tensor(score, dtype=torch.float64))


def test_rank_best_first_stable_and_inf_last():
    out = rescore.rank([_hyp(-3.0, 0), _hyp(float("-inf"), 1), _hyp(-1.0, 2), _hyp(-3.0, 3), _hyp(-2.0, 4)])
    assert [int(h.yseq[0]) for h in out] == [2, 4, 0, 3, 1]


class _HostSearch(rescore.CTCRescoringSearch):
    """the device stages replaced by host arithmetic: an "utterance" is a (T, 1) tensor whose
    first value v seeds the n-best [[v], [v, v + 1]]; token t scores -t (decoder), eos -0.5; the
    CTC nll of y is 2 * sum(y)"""

    def _ctc_logits(self, eng, xs):
        Ts = [int(x.shape[0]) for x in xs]
        return torch.stack(list(xs)), torch.zeros(len(xs) * max(Ts), 1), Ts, max(Ts)

    def _first_pass(self, eng, cl, Ts, Tm):
        return [[([int(v)], -1.0), ([int(v), int(v) + 1], -2.0)] for v in self.first]

    def _enqueue(self, eng, xu, clu, ys):
        L1 = max(len(y) for y in ys) + 1
        dec = torch.zeros(len(ys), L1)
        for b, y in enumerate(ys):
            dec[b, :len(y)] = -torch.tensor(y, dtype=torch.float32)
            dec[b, len(y)] = -0.5
        nll = torch.tensor([2.0 * sum(y) for y in ys])
        return torch.cat([dec.reshape(-1), nll]), dict(ys=ys, L1=L1, feas=[True] * len(ys))

    def decode_batch(self, xs):
        self.first = [float(x[0, 0]) for x in xs]
        return super().decode_batch(xs)


def test_plugs_into_run_sharded():
    """the object get_rescoring_decoder returns has decode_batch, so it is an infer_batch of
    evaluate.run_sharded as it stands; decode_batch's bookkeeping (one read for the batch, split
    back per utterance, fp64 score, ranking) on host stand-ins of the device stages"""
    s = _HostSearch(STUB, beam_size=2, ctc_weight=0.25)
    units = [torch.full((4, 1), float(v)) for v in (3, 5, 2, 7, 4)]

    def infer_batch(us):
        return [" ".join(TOKENS[t] for t in nbest[0].yseq.tolist()[1:-1]) for nbest in s.decode_batch(us)]

    texts = evaluate.run_sharded(units, None, infer_batch=infer_batch, batch=2)
    assert texts == ["u3", "u5", "u2", "u7", "u4"]          # [v] beats [v, v + 1] under these scores
    nbest = s.decode_batch(units[:1])[0]
    assert [h.yseq.tolist() for h in nbest] == [[V - 1, 3, V - 1], [V - 1, 3, 4, V - 1]]
    assert float(nbest[0].scores["decoder"]) == -3.5 and float(nbest[0].scores["ctc"]) == -6.0
    assert float(nbest[0].score) == 0.75 * -3.5 + 0.25 * -6.0
    assert float(nbest[1].score) == 0.75 * -7.5 + 0.25 * -14.0
    assert nbest[1].states["decoder"].tolist() == [-3.0, -4.0, -0.5]
    assert s(units[0])[0].yseq.tolist() == nbest[0].yseq.tolist()

"""Two-pass decoding on the HIP engine: CTC prefix beam search, then attention rescoring.

The joint search of avsr_amd.decode is label-synchronous: one decoder step (one read of all
decoder weights) per output token. This mode is the non-autoregressive route of the same joint
CTC / attention model:

  1. a time-synchronous CTC prefix beam search (avsr_ctc_beam, one launch for a batch of
     utterances) proposes an n-best list from the CTC posteriors alone;
  2. the attention decoder scores all candidates of an utterance in ONE teacher-forced pass
     (Engine.decoder_fwd, eval), and avsr_ctc_fwd gives each its exact CTC likelihood;
  3. the hypotheses are re-ranked by the joint score.

    search = get_rescoring_decoder(model.avsr, token_list, ctc_weight=0.1, beam_size=10)
    nbest = search(enc_out)                 # the reference's call form bs(x): List[Hypothesis]
    lists = search.decode_batch([enc_u for ...])

The reference has no such search; it does define the score. For a complete hypothesis y (ending
in eos) its joint search gives

    score(y) = (1 - w) * sum_j log p_dec(y_{j+1} | sos, y_1..y_j, x) + w * log p_ctc(y | x):

the per-step differences of CTCPrefixScorer telescope, and at eos they reach the full-sequence
probability (src/nets/ctc_prefix_score.py, src/nets/scorers/ctc.py). Every hypothesis returned
here carries exactly that score (and scores["decoder"], scores["ctc"]) — the score the
reference's search gives the same token sequence. ONLY THE CANDIDATE SET DIFFERS: it comes from
the CTC posteriors, not from the joint pre-beam. (One corner of the reference is not a complete
hypothesis in this sense: a hypothesis still running at maxlen gets eos APPENDED without a
score, batch_beam_search.py:320-330, so its decoder score has no eos term. The two-pass mode
always scores eos; Hypothesis.states["decoder"] holds the per-target log-probs, the last one
being that eos term.) How the mode's accuracy compares with the joint
search is not measured (no checkpoint or data here).

Shallow fusion (`set_lm`, avsr_amd/ngram_lm.py) adds to that score w_lm * the n-gram LM's log-prob
of y + [eos] from the <s> state and length_bonus * (len(y) + 1): one avsr_ngram_score_seqs launch
over an utterance's candidates in the second pass, the terms summed in fp64 on the host with the
others. The first pass is unchanged; every ctc_weight works (the terms are additive on complete
sequences). The effect on WER is unmeasured.
"""
from typing import List

import numpy as np
import torch

from . import ngram_lm
from . import ops
from .decode import Hypothesis

NEG_INF = float("-inf")


def ctc_feasible(T, y):
    """a CTC path for labels y over T frames exists iff T >= len(y) + the number of adjacent
    equal labels (each needs a blank between; avsr_ctc_align documents the same rule)"""
    y = [int(t) for t in y]
    return T >= len(y) + sum(a == b for a, b in zip(y, y[1:]))


def joint_score(dec_tokens, ctc, w):
    """(score, decoder, ctc) in fp64 from the fp32 per-token decoder log-probs (None: the decoder
    is not a scorer) and the fp32 CTC log-likelihood (None: CTC is not a scorer). The ends of the
    weight range use one scorer only, as the reference drops a scorer of weight 0."""
    dec = None if dec_tokens is None else float(np.sum(np.asarray(dec_tokens, dtype=np.float64)))
    ctc = None if ctc is None else float(ctc)
    if dec is None:
        return ctc, dec, ctc
    if ctc is None:
        return dec, dec, ctc
    return (1.0 - w) * dec + w * ctc, dec, ctc


def rank(hyps):
    """best first; equal scores keep their first-pass order (stable), -inf last"""
    return sorted(hyps, key=lambda h: -float(h.score))


def ctc_logits(eng, xs):
    """padded memory xp (U, Tm, D) in the engine dtype and CTC logits cl (U*Tm, Vp). The CTC
    head runs per utterance (M = T_u rows, as BatchBeamSearch.decode_batch does): the few-row
    and tiled GEMM cores round differently, so one launch over all U * Tm rows would make an
    utterance's result depend on the batch. (Shared with avsr_amd/confidence.py.)"""
    dev, D = eng.device, eng.dD
    Ts = [int(x.shape[0]) for x in xs]
    Tm = max(Ts + [1])
    xp = torch.zeros(len(xs), Tm, D, device=dev, dtype=eng.dtype)
    cl = torch.zeros(len(xs) * Tm, eng.Vp, device=dev, dtype=eng.dtype)
    for u, x in enumerate(xs):
        if Ts[u] == 0:
            continue
        ops.cast(x.to(dev).reshape(Ts[u], D).contiguous(), xp[u, :Ts[u]])
        ops.linear_fwd(xp[u, :Ts[u]], eng.w("ctc.ctc_lo.weight"), eng.arena.master("ctc.ctc_lo.bias"),
                       out=cl[u * Tm:u * Tm + Ts[u], :eng.V])
    return xp, cl, Ts, Tm


def decoder_token_logp(eng, xu, ys, sos, eos):
    """fp32 log-probabilities of the targets y + [eos] of each label sequence in ys under the
    attention decoder, for one utterance (xu (T, D) memory in the engine dtype): ONE
    teacher-forced pass over [sos] + y (rows padded with eos: the causal mask keeps earlier
    positions independent of the padding); targets y + [eos], -1 on padding (log-prob 0 there).
    Returns the device tensor (len(ys) * L1,), L1 = longest y + 1; nothing is read back. (The
    second pass of two-pass decoding and avsr_amd/confidence.py both score through this.)"""
    dev = eng.device
    T, n = int(xu.shape[0]), len(ys)
    L1 = max(len(y) for y in ys) + 1
    ys_in = torch.full((n, L1), eos, dtype=torch.int32)
    tgt = torch.full((n, L1), -1, dtype=torch.int32)
    for b, y in enumerate(ys):
        ys_in[b, 0] = sos
        ys_in[b, 1:len(y) + 1] = torch.tensor(y, dtype=torch.int32)
        tgt[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
        tgt[b, len(y)] = eos
    from .surface import _teacher_forced
    logits, _ = _teacher_forced(eng, ys_in.to(dev), xu.unsqueeze(0).expand(n, T, xu.shape[1]), None)
    return ops.token_logp(logits, eng.V, tgt.reshape(-1).to(dev))


class CTCRescoringSearch:
    """CTC prefix beam search (beam_size prefixes, token_beam candidate tokens per frame) and
    attention rescoring with the decoder + CTC scorers of an E2E model on its HIP engine."""

    def __init__(self, e2e, beam_size: int = 10, token_beam: int = None, ctc_weight: float = 0.1, sos: int = None,
                 eos: int = None, token_list: List[str] = None):
        if not 1 <= int(beam_size) <= ops.CTC_BEAM_MAX:
            raise ValueError(f"beam_size {beam_size} outside [1, {ops.CTC_BEAM_MAX}]")
        token_beam = min(int(beam_size), ops.CTC_BEAM_MAX) if token_beam is None else token_beam
        if not 1 <= int(token_beam) <= ops.CTC_BEAM_MAX:
            raise ValueError(f"token_beam {token_beam} outside [1, {ops.CTC_BEAM_MAX}]")
        if not 0.0 <= float(ctc_weight) <= 1.0:
            raise ValueError(f"ctc_weight {ctc_weight} outside [0, 1]")
        self.e2e = e2e
        self.beam_size, self.token_beam = int(beam_size), int(token_beam)
        self.ctc_weight = float(ctc_weight)
        self.sos = e2e.sos if sos is None else sos
        self.eos = e2e.eos if eos is None else eos
        self.blank = 0
        self.token_list = token_list
        self.use_dec, self.use_ctc = self.ctc_weight != 1.0, self.ctc_weight != 0.0
        self.lm, self.w_lm, self.w_len = None, 0.0, 0.0
        self._lm_dev = ngram_lm.FusionArrays()

    def __call__(self, x):
        return self.decode_batch([x])[0]

    def set_hotwords(self, phrases, bonus=None):
        """BatchBeamSearch.set_hotwords' call form: hot-word biasing lives in the joint search's
        step, so a phrase list is refused here; None / an empty list is accepted (nothing to clear)"""
        if phrases is not None and len(list(phrases)):
            raise NotImplementedError("hot words: the joint search only (get_beam_search_decoder)")

    def set_lm(self, lm, weight=0.0, length_bonus=0.0):
        """BatchBeamSearch.set_lm's call form: `lm` (an NgramLM over the model's token ids) at weight
        `weight` (finite, >= 0) and `length_bonus` (finite) per token of y + [eos], in the second
        pass; `set_lm(None, 0.0)` clears both"""
        V = None if self.token_list is None else len(self.token_list)
        self.lm, self.w_lm, self.w_len = ngram_lm.check_fusion(lm, weight, length_bonus, V, self.sos, self.eos)

    # ------------------------------------------------------------------- first pass
    def _ctc_logits(self, eng, xs):
        return ctc_logits(eng, xs)

    def _first_pass(self, eng, cl, Ts, Tm):
        """log-softmax + per-frame top token_beam of every row, then ONE avsr_ctc_beam launch for
        all utterances; one host read. -> per utterance [(tokens, search score)], best first"""
        U, dev = len(Ts), eng.device
        logp = torch.empty(U, Tm, eng.V, device=dev, dtype=torch.float32)
        cand = torch.empty(U, Tm, self.token_beam, device=dev, dtype=torch.int32)
        ops.log_softmax_topk(cl, eng.V, logp.view(U * Tm, eng.V), self.token_beam, cand.view(U * Tm, self.token_beam))
        n_out, tokens, length, score = ops.ctc_beam(logp, torch.tensor(Ts, dtype=torch.int32).to(dev), cand,
                                                    self.beam_size, blank=self.blank, eos=self.eos)
        n_out, tokens, length, score = (t.cpu().numpy() for t in (n_out, tokens, length, score))
        return [[(tokens[u, r, :length[u, r]].tolist(), float(score[u, r])) for r in range(int(n_out[u]))]
                for u in range(U)]

    @torch.no_grad()
    def ctc_nbest(self, xs):
        """the first pass alone: per encoded utterance (T_u, D) the kernel's n-best as
        [(tokens, ctc_search_score)], best first (tokens without sos / eos)"""
        if len(xs) == 0:
            return []
        eng = self.e2e.engine()
        _, cl, Ts, Tm = self._ctc_logits(eng, xs)
        return self._first_pass(eng, cl, Ts, Tm)

    # ------------------------------------------------------------------- second pass
    def _enqueue(self, eng, xu, clu, ys):
        """launch the scoring of label sequences ys for one utterance (xu (T, D) memory in the
        engine dtype, clu (T, Vp) its CTC logits); nothing is read back. Returns the device
        result [n * L1 decoder token log-probs | n CTC nll | n * L1 LM token scores], each part only
        for a scorer in use, and what _finish needs."""
        dev, V = eng.device, eng.V
        T, n = int(xu.shape[0]), len(ys)
        for y in ys:
            if any(t < 0 or t >= V for t in y):
                raise ValueError(f"token id outside [0, {V}): {y}")
            if self.use_ctc and any(t == self.blank or t == self.eos for t in y):
                raise ValueError(f"blank / eos are not CTC labels: {y}")
        Lmax = max(len(y) for y in ys)
        if Lmax > ops.CTC_BEAM_LCAP:
            raise ValueError(f"hypothesis of {Lmax} tokens: avsr_ctc_fwd scores at most {ops.CTC_BEAM_LCAP}")
        L1 = Lmax + 1
        parts = []
        if self.use_dec:
            parts.append(decoder_token_logp(eng, xu, ys, self.sos, self.eos))
        feas = [ctc_feasible(T, y) for y in ys]
        if self.use_ctc:
            # exact CTC likelihood of every hypothesis in ONE launch (the loss path's row-lse prologue
            # + avsr_ctc_fwd, one workgroup per hypothesis): the kernel addresses utterance b's
            # logits at rows b*T + t, so the utterance's logits and lse are repeated per hypothesis
            lse = torch.empty(T, device=dev, dtype=torch.float32)
            ops.row_lse(clu, V, lse)
            Lc = max(1, Lmax)
            lab = torch.full((n, Lc), -1, dtype=torch.int32)
            for b, y in enumerate(ys):
                lab[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
            llen = torch.tensor([len(y) for y in ys], dtype=torch.int32).to(dev)
            ilen = torch.full((n,), T, dtype=torch.int32).to(dev)
            alpha = torch.empty(n, T, 2 * Lc + 1, device=dev, dtype=torch.float32)
            gamma = torch.empty(n, T, 2 * Lc + 1, device=dev, dtype=torch.float32)
            nll = torch.zeros(n, device=dev, dtype=torch.float32)
            if T > 0:
                rep = clu.unsqueeze(0).expand(n, T, clu.shape[1]).reshape(n * T, clu.shape[1])
                ops.ctc_fwd(ops.ctc_params(rep, n, T, V, lab.to(dev), llen, ilen, lse.repeat(n), alpha, gamma, nll))
            parts.append(nll)
        if self.lm is not None:
            if self.lm.n_vocab != V:
                raise ValueError(f"the LM's vocabulary of {self.lm.n_vocab} is not the model's {V}")
            toks = torch.full((n, max(1, Lmax)), -1, dtype=torch.int32)
            for b, y in enumerate(ys):
                toks[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
            lm_out = ops.ngram_score_seqs(self._lm_dev.get(self.lm, dev), toks.to(dev), eos=self.eos)
            parts.append(lm_out[:, :L1].reshape(-1))
        return torch.cat(parts), dict(ys=ys, L1=L1, feas=feas)

    def _finish(self, res, meta):
        """host side: fp64 sums of the fp32 values, the joint score, the ranking"""
        ys, L1, n = meta["ys"], meta["L1"], len(meta["ys"])
        o = n * L1 if self.use_dec else 0
        dec = res[:o].reshape(n, L1) if self.use_dec else None
        nll = res[o:o + n] if self.use_ctc else None
        o += n if self.use_ctc else 0
        lms = res[o:o + n * L1].reshape(n, L1) if self.lm is not None else None
        hyps = []
        for b, y in enumerate(ys):
            # avsr_ctc_fwd implements zero_infinity: an infeasible pair comes back as nll 0
            ctc = None if nll is None else (-float(nll[b]) if meta["feas"][b] else NEG_INF)
            score, d, c = joint_score(None if dec is None else dec[b, :len(y) + 1], ctc, self.ctc_weight)
            scores, states = {}, {}
            if d is not None:
                scores["decoder"] = torch.tensor(d, dtype=torch.float64)
                # the fp32 log-prob of each of the L + 1 targets y + [eos], as the kernel gave them
                states["decoder"] = torch.from_numpy(np.array(dec[b, :len(y) + 1], dtype=np.float32))
            if c is not None:
                scores["ctc"] = torch.tensor(c, dtype=torch.float64)
            if lms is not None:
                # the fp32 LM score of each of the L + 1 tokens y + [eos], as the kernel gave them
                states["lm"] = torch.from_numpy(np.array(lms[b, :len(y) + 1], dtype=np.float32))
                lm_sum = float(np.sum(np.asarray(lms[b, :len(y) + 1], dtype=np.float64)))
                scores["lm"] = torch.tensor(lm_sum, dtype=torch.float64)
                score = score + self.w_lm * lm_sum
            if self.w_len != 0.0:
                scores["length_bonus"] = torch.tensor(float(len(y) + 1), dtype=torch.float64)
                score = score + self.w_len * float(len(y) + 1)
            hyps.append(Hypothesis(yseq=torch.tensor([self.sos] + list(y) + [self.eos], dtype=torch.int64),
                                   score=torch.tensor(score, dtype=torch.float64), scores=scores, states=states))
        return rank(hyps)

    @torch.no_grad()
    def rescore(self, x, yseqs) -> List[Hypothesis]:
        """the second pass alone: Hypotheses, best first, for one encoded utterance x (T, D) and
        label sequences yseqs (token ids without sos / eos)"""
        ys = [[int(t) for t in (y[0] if isinstance(y, tuple) and len(y) == 2 and isinstance(y[0], list) else y)]
              for y in yseqs]               # (tokens, score) pairs of ctc_nbest are taken as they come
        if not ys:
            return []
        if int(x.shape[0]) == 0:
            raise ValueError("rescore: an utterance of no frames")
        eng = self.e2e.engine()
        xp, cl, Ts, _ = self._ctc_logits(eng, [x])
        res, meta = self._enqueue(eng, xp[0, :Ts[0]], cl[:Ts[0]], ys)
        return self._finish(res.cpu().numpy(), meta)

    @torch.no_grad()
    def decode_batch(self, xs):
        """one n-best list per encoded utterance (T_u, D). The first pass is one launch for the
        batch; the decoder and CTC-likelihood passes run per utterance over that utterance's own
        hypotheses, so an utterance's result is identical whether it is decoded alone or in a
        batch (GEMM rounding depends on the row count). Two host reads per batch: the n-best
        of the first pass, and every utterance's scores together."""
        if len(xs) == 0:
            return []
        eng = self.e2e.engine()
        xp, cl, Ts, Tm = self._ctc_logits(eng, xs)
        nbest = self._first_pass(eng, cl, Ts, Tm)
        queued = []
        for u, nb in enumerate(nbest):
            ys = [y for y, _ in nb]
            queued.append(self._enqueue(eng, xp[u, :Ts[u]], cl[u * Tm:u * Tm + Ts[u]], ys) if ys else None)
        live = [q for q in queued if q is not None]
        if not live:
            return [[] for _ in xs]
        host = torch.cat([r for r, _ in live]).cpu().numpy()
        out, o = [], 0
        for q in queued:
            if q is None:
                out.append([])
                continue
            k = q[0].numel()
            out.append(self._finish(host[o:o + k], q[1]))
            o += k
        return out


def get_rescoring_decoder(model, token_list, ctc_weight=0.1, beam_size=10, token_beam=None, hotwords=None,
                          hotword_bonus=None, lm=None, lm_weight=0.0, length_bonus=0.0):
    """the two-pass counterpart of get_beam_search_decoder — `model` is the E2E
    (`AVHubertAVSR.avsr`); the result has the same call forms (bs(x), decode_batch(xs)). A hot-word
    list is refused (NotImplementedError): biasing is part of the joint search only. lm (an NgramLM),
    lm_weight and length_bonus: `set_lm` on the result"""
    search = CTCRescoringSearch(model, beam_size=beam_size, token_beam=token_beam, ctc_weight=ctc_weight,
                                sos=model.sos, eos=model.eos, token_list=token_list)
    search.set_hotwords(hotwords, hotword_bonus)
    search.set_lm(lm, lm_weight, length_bonus)
    return search

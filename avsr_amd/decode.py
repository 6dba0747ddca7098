"""Joint CTC / attention beam search on the HIP engine.

Drop-in for the decoder the reference builds with `get_beam_search_decoder`
(src/avhubert_avsr/avhubert_avsr_model.py:12-36): a `BatchBeamSearch` whose call
`bs(x)` on one encoded utterance x (T, d) returns the ended hypotheses sorted by score,
`Hypothesis.asdict()["yseq"]` starting with sos (script/evaluation.py:104-107).

Search semantics follow src/nets/batch_beam_search.py:102-349 and beam_search.py:330-456
(weights decoder 1-ctc_weight / ctc ctc_weight, length bonus and LM weight 0 => dropped,
pre-beam of int(1.5*beam) tokens on the decoder score, maxlen = T when maxlenratio = 0,
eos forced at the last step, end detection M=3, D_end=-10). Everything runs on the device,
bookkeeping included (decoder one-step with an ancestry-indexed self-attention K/V cache and
per-utterance cross-attention K/V, pre-beam top-k, CTC prefix recursion, weighted flat
top-beam, running scores, back-pointers, ended-hypothesis records, end detection), and every
step after the first is one HIP-graph replay; the host reads a finished-utterance count every
8 steps and the history once at the end — the reference synchronises per hypothesis.
The step's kernels, one family per file of csrc/: decode_softmax.hip (log-softmax, top-k),
dec_attn.hip, ctc_prefix.hip, beam.hip (selection, bookkeeping, state gather), and hotword.hip /
ngram.hip for the two optional scorers below.

A stream of utterances of unequal length goes through a `DecodeSession` (`bs.stream()`,
`bs.decode_stream(xs)`): a fixed number of utterance slots whose graphs are captured once, a
finished utterance's slot refilled with the next input while the others keep stepping
(continuous batching). There the position is kept per row, not once for the batch.

Differences that do not change results: the cross-attention K/V of the memory are computed
once per utterance (the reference recomputes them every step), the self-attention K/V of
earlier positions are cached instead of the layer outputs they are computed from (rows of
step j at cache row j*R + r, reached through each hypothesis's ancestry table instead of
being copied on every reorder), and finished hypotheses stay in the batch as dead rows.

The two ends of the CTC-weight range are the configurations the reference builds with one
scorer (a scorer of weight 0 is dropped, beam_search.py:69-73): ctc_weight = 0 searches on the
decoder alone (no partial scorer, so no pre-beam: every token of every row is a candidate);
ctc_weight = 1 on the CTC prefix scorer alone over the full vocabulary (pre_beam_score_key None,
no decoder step at all): psi of every token in chunks of 64, then the row's top int(1.5*beam)
tokens by psi (a superset of every token the flat top-beam can pick from that row, since the row
offset is common) get their CTC states.

Hot-word biasing (`set_hotwords`, avsr_amd/hotwords.py; the joint search through `bs(x)` and
`decode_batch` only) is the one way this search takes information from outside the model: the
reference plugs host scorers into its loop, a replayed graph has no host in its loop, so the bias
is a kernel of the step. Every row carries a node of the phrases' prefix tree; after the pre-beam
`ops.hotword_step` widens the row's candidates by the next tokens of a phrase it is inside (at most
8 more columns, which get real CTC prefix scores) and gives every candidate column its bonus and
successor node; `beam_select` adds the bonus between the CTC term and the running score, `beam_post`
sums it in fp64 (`Hypothesis.scores["hotword"]`) and writes the selected successor into the other
node buffer. Phrase starts are rewarded only when the decoder's pre-beam holds them. A hypothesis
the length limit closes keeps the bonus of a phrase it had not finished: the reference appends that
eos without scoring it, so nothing cancels there. With no phrase list none of this is allocated or
launched.

Shallow fusion with a token-level n-gram LM and the length bonus (`set_lm`, avsr_amd/ngram_lm.py;
the "lm" and "length_bonus" slots of the reference's scorer dict, which it hard-wires off) follow
the same route: every row carries a state of the LM's backoff automaton, `ops.ngram_step` scores
the row's (widened) candidate columns and eos after the pre-beam, `beam_select` adds
w_len + w_lm * lm in the reference's summation order (full scorers, then partial scorers, then the
running score), `beam_post` sums both in fp64 (`Hypothesis.scores["lm"]`, the unweighted sum, and
`scores["length_bonus"]`, the number of scored tokens) and writes the successor state into the other
state buffer. Same scope as hot words: the joint search through `bs(x)` and `decode_batch`; with
neither set nothing of it is allocated or launched.
"""
import math
from typing import Any, Dict, List, NamedTuple, Union

import numpy as np
import torch

from . import hotwords
from . import ngram_lm
from . import ops
from . import stream_slots

LOGZERO = -10000000000.0
# fp32 decode: LayerNorms folded into the linears they feed (the few-row kernel's LN prologue)
FOLD_LN = True
D_END = np.log(1 * np.exp(-10))          # end_detect's threshold (e2e_asr_common.py:18)


class Hypothesis(NamedTuple):
    """src/nets/beam_search.py:13-29"""
    yseq: torch.Tensor
    score: Union[float, torch.Tensor] = 0
    scores: Dict[str, Union[float, torch.Tensor]] = dict()
    states: Dict[str, Any] = dict()

    def asdict(self) -> dict:
        return self._replace(
            yseq=self.yseq.tolist(),
            score=float(self.score),
            scores={k: float(v) for k, v in self.scores.items()},
        )._asdict()


def end_detect(ended_hyps, i, M=3, D_end=D_END):
    """src/nets/e2e_asr_common.py:18-48 (host form; the search evaluates it on the device,
    beam.hip beam_post_kernel, over the per-length best ended scores)"""
    if len(ended_hyps) == 0:
        return False
    count = 0
    best_hyp = sorted(ended_hyps, key=lambda x: x["score"], reverse=True)[0]
    for m in range(M):
        hyp_length = i - m
        same = [x for x in ended_hyps if len(x["yseq"]) == hyp_length]
        if len(same) > 0:
            best_same = sorted(same, key=lambda x: x["score"], reverse=True)[0]
            if best_same["score"] - best_hyp["score"] < D_end:
                count += 1
    return count == M


_CAPTURE_STREAMS = {}


def _capture_stream(dev):
    """one graph-capture stream per device for every search (its workspaces are reused)"""
    s = _CAPTURE_STREAMS.get(dev)
    if s is None:
        s = _CAPTURE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return s


class BatchBeamSearch:
    """Beam search over one utterance with the decoder + CTC prefix scorers of an E2E model
    running on its HIP engine."""

    def __init__(self, e2e, beam_size: int, vocab_size: int, weights: Dict[str, float], sos: int, eos: int,
                 token_list: List[str] = None, pre_beam_ratio: float = 1.5, pre_beam_score_key: str = "decoder"):
        self.e2e = e2e
        self.beam_size = beam_size
        self.n_vocab = vocab_size
        self.weights = weights
        self.sos, self.eos = sos, eos
        self.blank = 0
        self.token_list = token_list
        self.pre_beam_size = int(pre_beam_ratio * beam_size)
        self.w_dec = float(weights.get("decoder", 0.0))
        self.w_ctc = float(weights.get("ctc", 0.0))
        self.use_dec, self.use_ctc = self.w_dec != 0.0, self.w_ctc != 0.0
        if not (self.use_dec or self.use_ctc):
            raise NotImplementedError("no scorer with a non-zero weight")
        if self.use_ctc and pre_beam_score_key is not None and pre_beam_score_key != "decoder":
            raise NotImplementedError(f"pre-beam on {pre_beam_score_key!r}: the reference builds 'decoder' or None")
        if self.use_ctc and not self.use_dec and pre_beam_score_key == "decoder":
            raise KeyError("decoder is not a scorer (weight 0): pre_beam_score_key must be None")   # beam_search.py:92-97
        if self.use_ctc and self.use_dec and (pre_beam_score_key is None or not self.pre_beam_size < vocab_size):
            raise NotImplementedError("the joint search pre-beams on the decoder score, as the reference configures it")
        self.hotwords, self.hotword_bonus = None, None
        self._hotword_dev = {}
        self.lm, self.w_lm, self.w_len = None, 0.0, 0.0
        self._lm_dev = ngram_lm.FusionArrays()

    # ----------------------------------------------------------------------- hot words
    def set_hotwords(self, phrases, bonus=None):
        """Bias the search towards `phrases` (lists of token ids, see avsr_amd.hotwords): every
        token that continues a phrase adds `bonus` (> 0, no default: a tuning knob nobody has
        measured for this model) to the hypothesis score, a phrase left unfinished gives it back.
        `set_hotwords(None)` or an empty list clears the list: the search then launches exactly what
        it launches without this feature. The joint search only (0 < ctc_weight < 1), through
        `bs(x)` and `decode_batch`."""
        phrases = None if phrases is None else list(phrases)
        if not phrases:
            self.hotwords, self.hotword_bonus, self._hotword_dev = None, None, {}
            return
        if not (self.use_dec and self.use_ctc):
            raise NotImplementedError("hot words: the joint search only (0 < ctc_weight < 1)")
        if bonus is None or not float(bonus) > 0.0 or not math.isfinite(float(bonus)):
            raise ValueError(f"hot words need a per-token bonus > 0 (got {bonus!r})")
        tree = hotwords.build_tree(phrases, eos=self.eos, blank=self.blank)
        if max(int(tree.child_tok.max()), 0) >= self.n_vocab:
            raise ValueError(f"a phrase holds a token id outside the vocabulary of {self.n_vocab}")
        self.hotwords, self.hotword_bonus, self._hotword_dev = tree, float(bonus), {}

    def _hotword_arrays(self, dev):
        """the tree's flat arrays on `dev` (uploaded once per device and phrase list)"""
        key = str(dev)
        if key not in self._hotword_dev:
            t = self.hotwords
            self._hotword_dev[key] = {k: torch.from_numpy(getattr(t, k)).to(dev) for k in
                                      ("child_off", "child_tok", "child_node", "pend", "terminal")}
        return self._hotword_dev[key]

    # ----------------------------------------------------------------------- LM shallow fusion
    def set_lm(self, lm, weight=0.0, length_bonus=0.0):
        """Shallow fusion with `lm` (an avsr_amd.ngram_lm.NgramLM over this search's token ids) at
        weight `weight` (finite, >= 0), and `length_bonus` (finite) added per scored token, which may
        be set alone: score = (1-w)*dec + w*ctc + weight*lm + length_bonus*len [+ hotword]. Good
        values of either are unmeasured for this model. `set_lm(None, 0.0)` clears both: the search
        then launches exactly what it launches without this feature. The joint search only
        (0 < ctc_weight < 1), through `bs(x)` and `decode_batch`."""
        lm, weight, length_bonus = ngram_lm.check_fusion(lm, weight, length_bonus, self.n_vocab, self.sos, self.eos)
        if (lm is not None or length_bonus != 0.0) and not (self.use_dec and self.use_ctc):
            raise NotImplementedError(
                "LM fusion / length bonus: the joint search only (0 < ctc_weight < 1); at ctc_weight 0 or 1 every "
                "vocabulary entry is a candidate, which would need a V-wide LM pass. Use a ctc_weight inside (0, 1), "
                "or the two-pass decoder (get_rescoring_decoder), which takes an LM at every ctc_weight")
        self.lm, self.w_lm, self.w_len = lm, weight, length_bonus
        self.weights = {**self.weights, "lm": self.w_lm, "length_bonus": self.w_len}

    def __call__(self, x, maxlenratio: float = 0.0, minlenratio: float = 0.0):
        return self.forward(x, maxlenratio, minlenratio)

    def _cross_group(self, Tm):
        """hypotheses of one utterance per cross-attention workgroup: the beam, while its
        [beam][Tm] scores fit the grouped kernel's LDS (about 2.7 k frames at beam 5)"""
        G = self.beam_size if self.beam_size <= 8 else 1
        return G if ops.dec_attn_group_fits(Tm, G) else 1

    # ----------------------------------------------------------------------- decoder step
    def _decoder_step(self, eng, st):
        """Decoder.forward_one_step for the R rows of the search state `st` (position and
        tokens on the device): returns log-probs (R, V) fp32. This step's self-attention K / V
        go to cache rows pos*R + r; key j of row r is cache row anc[r][j] (its ancestry), the
        memory of row r is utterance r // beam over klen[r] frames."""
        ar = eng.arena
        D, H, R = eng.dD, eng.dH, st["R"]
        pos, cache, anc = st["pos"], st["cache"], st["anc_in"]
        pr = st["per_row"]                      # a session's state: pos holds one position per row
        x = eng._e(R, D)
        ops.embed_fwd(st["tok"], eng.w("decoder.embed.0.weight"), eng._pe, math.sqrt(D), x, 1, pe_row=pos, per_row=pr)
        Tm = st["Tm"]
        fold = st.get("fold")
        for i in range(eng.dl):
            p = f"decoder.decoders.{i}."
            sa, ca, ff = p + "self_attn.", p + "src_attn.", p + "feed_forward."
            kc, vc = cache[i, 0], cache[i, 1]               # (Lmax * R, D): rows step * R + r
            if fold is not None:       # norm1 folded into the QKV linear, K / V appended to the cache (one launch)
                Wg, bb, c1 = fold[i]["qkv"]
                qkv = ops.linear_fwd(x, Wg, bb, ln=(c1, 1e-12), kv=(kc, vc, pos, R, pr))
            else:
                n1, _, _ = ops.layernorm_fwd(x, ar.master(p + "norm1.weight"), ar.master(p + "norm1.bias"), 1e-12)
                qkv = ops.linear_fwd(n1, ar.span([sa + "linear_q.weight", sa + "linear_k.weight", sa + "linear_v.weight"]),
                                     ar.span([sa + "linear_q.bias", sa + "linear_k.bias", sa + "linear_v.bias"],
                                             buf="master"))
                ops.beam_kv_put(qkv, kc, vc, pos, R, D, per_row=pr)
            o1 = eng._e(R, D)
            ops.dec_attn(qkv[:, :D], kc, vc, o1, n=R, H=H, klen_max=st["Lmax"], k_bstride=0, v_bstride=0,
                         klen=st["klen_self"], kmap=anc)
            y1 = ops.linear_fwd(o1, eng.w(sa + "linear_out.weight"), ar.master(sa + "linear_out.bias"), res=x)
            if fold is not None:
                Wg, bb, c1 = fold[i]["q2"]
                q2 = ops.linear_fwd(y1, Wg, bb, ln=(c1, 1e-12))
            else:
                n2, _, _ = ops.layernorm_fwd(y1, ar.master(p + "norm2.weight"), ar.master(p + "norm2.bias"), 1e-12)
                q2 = ops.linear_fwd(n2, eng.w(ca + "linear_q.weight"), ar.master(ca + "linear_q.bias"))
            o2 = eng._e(R, D)
            kv = st["mem"][i]
            ops.dec_attn(q2, kv[:, :D], kv[:, D:], o2, n=R, H=H, klen_max=Tm, k_bstride=Tm * kv.stride(0),
                         v_bstride=Tm * kv.stride(0), kidx=st["uidx"], klen=st["klen_mem"],
                         group=self._cross_group(Tm), ksplit=2)
            y2 = ops.linear_fwd(o2, eng.w(ca + "linear_out.weight"), ar.master(ca + "linear_out.bias"), res=y1)
            if fold is not None:
                Wg, bb, c1 = fold[i]["ff1"]
                a = ops.linear_fwd(y2, Wg, bb, act=ops.L.ACT_RELU, ln=(c1, 1e-12))
            else:
                n3, _, _ = ops.layernorm_fwd(y2, ar.master(p + "norm3.weight"), ar.master(p + "norm3.bias"), 1e-12)
                a = ops.linear_fwd(n3, eng.w(ff + "w_1.weight"), ar.master(ff + "w_1.bias"), act=ops.L.ACT_RELU)
            x = ops.linear_fwd(a, eng.w(ff + "w_2.weight"), ar.master(ff + "w_2.bias"), res=y2)
        yn, _, _ = ops.layernorm_fwd(x, ar.master("decoder.after_norm.weight"), ar.master("decoder.after_norm.bias"),
                                     1e-12)
        logits = eng._e(R, eng.Vp)
        ops.linear_fwd(yn, eng.w("decoder.output_layer.weight"), ar.master("decoder.output_layer.bias"),
                       out=logits[:, :eng.V])
        logp = torch.empty(R, eng.V, device=eng.device, dtype=torch.float32)
        # log-probs and the pre-beam (top-P decoder tokens per row) in one pass
        return ops.log_softmax_topk(logits, eng.V, logp, self.pre_beam_size, st["ids"])

    def _fold_layernorms(self, eng):
        """fp32 decode: each decoder layer's norm1 / norm2 / norm3 folded into the linear it feeds
        (QKV, cross-attention query, FFN w_1): ops.fold_layernorm weights for the few-row kernel's
        LayerNorm prologue (one launch instead of two per pair). Prepared per search (the weights may
        have changed since the last one); None where the prologue does not apply (bf16, D > 1024)."""
        if eng.dtype != torch.float32 or eng.dD > 1024 or eng.dD % 16:
            return None
        ar = eng.arena
        out = []
        for i in range(eng.dl):
            p = f"decoder.decoders.{i}."
            sa, ca, ff = p + "self_attn.", p + "src_attn.", p + "feed_forward."

            def f(W, b, n):
                return ops.fold_layernorm(W, b, ar.master(n + ".weight"), ar.master(n + ".bias"))
            out.append(dict(
                qkv=f(ar.span([sa + "linear_q.weight", sa + "linear_k.weight", sa + "linear_v.weight"]),
                      ar.span([sa + "linear_q.bias", sa + "linear_k.bias", sa + "linear_v.bias"], buf="master"),
                      p + "norm1"),
                q2=f(eng.w(ca + "linear_q.weight"), ar.master(ca + "linear_q.bias"), p + "norm2"),
                ff1=f(eng.w(ff + "w_1.weight"), ar.master(ff + "w_1.bias"), p + "norm3")))
        return out

    def _ctc_full_vocab(self, st, r_prev, ctc_kw):
        """ctc_weight = 1: psi of every token (chunks of 64 ids through the prefix kernel, ctc_kw the
        step's ctc_prefix keywords), then the row's top-P tokens by psi into st["ids"] (the kernel's
        psi of a token does not depend on the other ids of its launch)"""
        pf = st["psi_full"]
        for c in range(st["vchunks"].shape[0]):
            ops.ctc_prefix(st["logp"], r_prev, st["tok"], st["vchunks"][c], st["r_scr"], st["psi_c"], **ctc_kw)
            pf[:, c * 64:(c + 1) * 64].copy_(st["psi_c"][:, :64])
        ops.row_topk(pf, self.n_vocab, self.pre_beam_size, st["ids"])

    def _step(self, eng, st, first, k):
        """one search step on the device (no host sync): decoder, pre-beam, CTC prefix scores,
        per-utterance beam selection, bookkeeping, state reorder. k = 0 / 1 picks the ancestry
        and CTC-state ping-pong buffers (read k, write 1 - k)."""
        R, P, beam = st["R"], self.pre_beam_size, self.beam_size
        st["anc_in"] = st["anc"][k]
        ops.beam_step_prep(R, st["pos"], st["anc"][k], st["klen_self"], per_row=st["per_row"])
        # decoder log-probs + the pre-beam ids; without a decoder scorer its score is 0
        dec = self._decoder_step(eng, st) if self.use_dec else st["dec0"]
        # sel_extra / post_extra: what hot words, the LM and the length bonus add to beam_select / beam_post
        ids, hw, sel_extra, post_extra = st["ids"], st.get("hw"), {}, {}
        if hw is not None:
            # hot words: the candidates widen by the continuations of each row's tree node; bonus and
            # successor node per column (node ping-pong: read k, beam_post writes 1 - k)
            ids = hw["ids"]
            ops.hotword_step(hw["tree"], hw["node"][k], st["ids"], ids, hw["bonus"], hw["next"], beta=hw["beta"],
                             blank=self.blank, eos=self.eos)
            P = ids.shape[1]
            sel_extra = dict(bonus=hw["bonus"], nxt=hw["next"])
        lm = st.get("lm")
        if lm is not None and "arrays" in lm:
            # the LM scores the widened ids (continuation columns too) and eos from each row's state
            # (state ping-pong: read k, beam_post writes 1 - k)
            ops.ngram_step(lm["arrays"], lm["state"][k], ids, lm["score"], lm["next"], blank=self.blank, eos=self.eos)
            sel_extra.update(lm=lm["score"], lm_next=lm["next"], w_lm=self.w_lm, lm_hi=lm["arrays"]["lm_hi"])
        if lm is not None:
            sel_extra["w_len"] = self.w_len
        if self.use_ctc:
            r_prev = None if first else st["r_prev"][k]
            ctc_kw = dict(n=R, out_len=0, out_len_dev=st["pos"], per_row=st["per_row"], blank=self.blank, eos=self.eos,
                          uidx=st["uidx"], tlen=st["tlen"])
            if not self.use_dec:
                self._ctc_full_vocab(st, r_prev, ctc_kw)
            ops.ctc_prefix(st["logp"], r_prev, st["tok"], ids, st["r_new"], st["psi"], **ctc_kw)
        out = st["out"]
        ops.beam_select(dec, self.n_vocab, ids, st["psi"], st["s_prev"], st["score"], out, n=R, beam=beam,
                        blank=self.blank, eos=self.eos, w_dec=self.w_dec, w_ctc=self.w_ctc, seg=st["seg"], **sel_extra)
        if hw is not None:
            post_extra = dict(sel_bonus=out["bonus"], sel_next=out["next"], shw=hw["shw"], end_hw=hw["end_hw"],
                              node_out=hw["node"][1 - k])
        if lm is not None and "arrays" in lm:
            post_extra.update(sel_lm=out["lm"], sel_lm_next=out["lm_next"], slm=lm["slm"], end_lm=lm["end_lm"],
                              lm_state_out=lm["state"][1 - k], lm_start=lm["arrays"]["start"])
        if lm is not None and "slen" in lm:
            post_extra.update(slen=lm["slen"], end_len=lm["end_len"])
        ops.beam_post(U=st["U"], beam=beam, P=P, R=R, Lmax=st["Lmax"], steps_cap=st["steps"], eos=self.eos,
                      end_detect=st["end_detect"], d_end=float(D_END), pos=st["pos"], maxlen=st["maxlen"],
                      sel_prev=out["prev"], sel_tok=out["tok"], sel_col=out["col"], sel_score=out["score"],
                      sel_dec=out["dec"], sel_ctc=out["ctc"], sel_s=out["s"], tok=st["tok"], score=st["score"],
                      sdec=st["sdec"], sctc=st["sctc"], s_prev=st["s_prev"], src=st["src"], bp_prev=st["bp_prev"],
                      bp_tok=st["bp_tok"], end_flag=st["end_flag"], end_score=st["end_score"], end_dec=st["end_dec"],
                      end_ctc=st["end_ctc"], best_len=st["best_len"], best_end=st["best_end"], done=st["done"],
                      upos=st.get("upos"), rowpos=st.get("rowpos"), **post_extra)
        Lm, Tm = st["Lmax"], st["Tm"]
        ops.gather_rows(st["anc"][k], st["anc"][1 - k], st["src"][:R], groups=1, n=R, row_bytes=Lm * 4,
                        src_gstride=0, src_rstride=Lm * 4, dst_gstride=0, dst_rstride=Lm * 4)
        if self.use_ctc:
            ops.gather_rows(st["r_new"], st["r_prev"][1 - k], st["src"][R:], groups=1, n=R, row_bytes=Tm * 2 * 4,
                            src_gstride=0, src_rstride=Tm * 2 * 4, dst_gstride=0, dst_rstride=Tm * 2 * 4)

    # ----------------------------------------------------------------------- search
    def forward(self, x, maxlenratio: float = 0.0, minlenratio: float = 0.0) -> List[Hypothesis]:
        """the reference's call form bs(x) on one encoded utterance (T, d)"""
        return self.decode_batch([x], maxlenratio, minlenratio)[0]

    def decode_batch(self, xs, maxlenratio: float = 0.0, minlenratio: float = 0.0):
        """Beam search of U utterances at once: xs = list of encoded utterances (T_u, d). Per
        utterance the search is exactly `self(x)` of the reference (batch_beam_search.py:102-349,
        beam_search.py:330-456): same scores, same stopping rules (maxlen = T_u, end detection,
        eos forced at the last step). The whole search state lives on the device in a fixed
        geometry of U x beam rows (a finished hypothesis or utterance becomes a dead row with
        score -inf, which no selection picks — the same outcome as the reference removing it);
        the first step runs eagerly, every later step is ONE replay of a captured HIP graph (two
        graphs: the ancestry / CTC-state ping-pong buffers alternate), the host only reads the
        count of finished utterances every few steps and the history once at the end. Returns
        one n-best list per utterance."""
        eng = self.e2e.engine()
        dev = eng.device
        U = len(xs)
        if U == 0:
            return []
        Ts = [int(x.shape[0]) for x in xs]
        Tm = max(Ts)
        maxlens = [self._maxlen(T, maxlenratio) for T in Ts]
        D = eng.dD
        # padded memory [U][Tm][D] -> CTC log-probs [U][Tm][V] and per-layer cross K/V [U*Tm][2D]
        xp = torch.zeros(U, Tm, D, device=dev, dtype=eng.dtype)
        for u, x in enumerate(xs):      # (the cast kernel converts fp32 encoder outputs to bf16 if needed)
            ops.cast(x.to(dev).reshape(Ts[u], D).contiguous(), xp[u, :Ts[u]])
        cl = torch.zeros(U * Tm, eng.Vp, device=dev, dtype=eng.dtype)
        mem = [torch.zeros(U * Tm, 2 * D, device=dev, dtype=eng.dtype) for _ in range(eng.dl)]
        for u in range(U):
            self._project_memory(eng, xp[u, :Ts[u]], cl[u * Tm:u * Tm + Ts[u]], mem, u * Tm)
        # one log-softmax over all U * Tm rows: the padding rows (zero logits) get finite log-probs
        logp = torch.empty(U, Tm, eng.V, device=dev, dtype=torch.float32)
        ops.log_softmax_rows(cl, eng.V, logp.view(U * Tm, eng.V))
        steps = max(maxlens)
        eng.ensure_pe(steps + 1)
        st = self._new_state(dev, eng.dtype, Ts, maxlens, logp, mem, D, eng.dl, end_detect=int(maxlenratio == 0.0),
                             fold=self._fold_layernorms(eng) if FOLD_LN and self.use_dec else None)
        self._step(eng, st, True, 0)           # step 0: CTC state from scratch; reads ancestry 0, writes 1
        if steps > 1:
            graphs = self._capture(eng, st)
            done_host = st["done"][U:]
            for i in range(1, steps):
                graphs[i & 1].replay()         # step i reads ping-pong buffer i & 1
                if i % 8 == 0 and int(done_host.item()) == U:
                    break
        torch.cuda.current_stream(dev).synchronize()
        return self._collect(st, xs, maxlenratio, minlenratio)

    def _project_memory(self, eng, xu, cl, mem, r0):
        """The CTC head and the cross-attention K / V projections of one utterance xu (T, D), already
        cast to the engine's dtype: logits into cl (its T rows), layer i's K / V into
        mem[i][r0:r0 + T]. Per utterance (M = T rows, as in the one-utterance call): the few-row and
        tiled GEMM cores round differently, so one launch over all rows of a batch would make an
        utterance's scores depend on the batch. The log-softmax stays with the caller: decode_batch
        runs one over the rows of all utterances, a session one over the slot's T rows."""
        ar, T = eng.arena, xu.shape[0]
        ops.linear_fwd(xu, eng.w("ctc.ctc_lo.weight"), ar.master("ctc.ctc_lo.bias"), out=cl[:, :eng.V])
        for i in range(eng.dl):
            ca = f"decoder.decoders.{i}.src_attn."
            ops.linear_fwd(xu, ar.span([ca + "linear_k.weight", ca + "linear_v.weight"]),
                           ar.span([ca + "linear_k.bias", ca + "linear_v.bias"], buf="master"), out=mem[i][r0:r0 + T])

    def _new_state(self, device, dtype, Ts, maxlens, logp, mem, D, layers, end_detect=1, fold=None):
        """the device-side search state of U = len(Ts) utterances (Ts frames, maxlens steps each)
        before step 0: one live hypothesis (sos) per utterance. logp (U, Tm, V) fp32 CTC log-probs,
        mem per decoder layer the cross-attention K/V [U*Tm][2D]; the self-attention cache is
        (layers, 2, Lmax*R, D) of `dtype`. Depends on no engine, so a search whose
        `_decoder_step` is replaced (the scripted-decoder tests) builds it too."""
        dev = device
        U, Tm, V = len(Ts), max(Ts), logp.shape[-1]
        P, beam = self.pre_beam_size, self.beam_size
        steps = max(maxlens)
        Lmax = steps + 1
        R = U * beam
        i32 = dict(device=dev, dtype=torch.int32)
        f32 = dict(device=dev, dtype=torch.float32)
        f64 = dict(device=dev, dtype=torch.float64)
        rows = torch.arange(R, dtype=torch.int32)
        score0 = torch.full((R,), float("-inf"))
        score0[::beam] = 0.0                  # one live hypothesis (sos) per utterance
        st = dict(
            U=U, R=R, Lmax=Lmax, Tm=Tm, steps=steps, end_detect=int(end_detect), mem=mem, logp=logp, per_row=False,
            pos=torch.zeros(1, **i32), maxlen=torch.tensor(maxlens, dtype=torch.int32).to(dev),
            tok=torch.full((R,), self.sos, **i32), score=score0.to(dev),
            sdec=torch.zeros(R, **f64), sctc=torch.zeros(R, **f64), s_prev=torch.zeros(R, **f32),
            cache=torch.empty(layers, 2, Lmax * R, D, device=dev, dtype=dtype),
            anc=[torch.zeros(R, Lmax, **i32), torch.zeros(R, Lmax, **i32)], klen_self=torch.empty(R, **i32),
            uidx=(rows // beam).to(dev), klen_mem=torch.tensor(Ts, dtype=torch.int32)[rows // beam].to(dev),
            tlen=torch.tensor(Ts, dtype=torch.int32).to(dev),
            seg=(torch.arange(U + 1, dtype=torch.int32) * beam).to(dev),
            ids=torch.empty(R, P, **i32), psi=torch.empty(R, P + 1, **f32),
            r_new=torch.empty(R, P, Tm, 2, **f32), r_prev=[torch.empty(R, Tm, 2, **f32), torch.empty(R, Tm, 2, **f32)],
            out={**{k: torch.empty(R, **i32) for k in ("prev", "tok", "col")},
                 **{k: torch.empty(R, **f32) for k in ("score", "dec", "ctc", "s")}},
            src=torch.empty(2 * R, **i32),
            bp_prev=torch.zeros(steps, R, **i32), bp_tok=torch.zeros(steps, R, **i32),
            end_flag=torch.zeros(steps, R, **i32), end_score=torch.zeros(steps, R, **f32),
            end_dec=torch.zeros(steps, R, **f64), end_ctc=torch.zeros(steps, R, **f64),
            best_len=torch.full((U, Lmax + 3), float("-inf"), **f32), best_end=torch.full((U,), float("-inf"), **f32),
            done=torch.zeros(U + 1, **i32), fold=fold)
        if self.hotwords is not None:
            # hot words: candidates, CTC scores and states over Pw = P + C columns (st["ids"] stays
            # the pre-beam the decoder step writes), the per-column bonus / successor node, the
            # node of every row (root for sos; ping-pong like anc), the bonus sums and their history
            Pw = P + hotwords.MAX_CHILDREN
            st["psi"] = torch.empty(R, Pw + 1, **f32)
            st["r_new"] = torch.empty(R, Pw, Tm, 2, **f32)
            st["out"]["bonus"], st["out"]["next"] = torch.empty(R, **f32), torch.empty(R, **i32)
            st["hw"] = dict(tree=self._hotword_arrays(dev), beta=self.hotword_bonus,
                            ids=torch.empty(R, Pw, **i32), bonus=torch.empty(R, Pw + 1, **f32),
                            next=torch.empty(R, Pw + 1, **i32), node=[torch.zeros(R, **i32), torch.zeros(R, **i32)],
                            shw=torch.zeros(R, **f64), end_hw=torch.zeros(steps, R, **f64))
        if self.lm is not None or self.w_len != 0.0:
            # LM fusion / length bonus: the LM state of every row (<s> for sos; ping-pong like anc), the
            # per-column score / successor over the (widened) candidate columns, the fp64 sums and
            # their history; each only for a scorer of non-zero weight
            lm = st["lm"] = {}
            if self.lm is not None:
                arr = self._lm_dev.get(self.lm, dev)
                Wc = st["psi"].shape[1]
                st["out"]["lm"], st["out"]["lm_next"] = torch.empty(R, **f32), torch.empty(R, **i32)
                lm.update(arrays=arr, state=[torch.full((R,), arr["start"], **i32) for _ in range(2)],
                          score=torch.empty(R, Wc, **f32), next=torch.empty(R, Wc, **i32),
                          slm=torch.zeros(R, **f64), end_lm=torch.zeros(steps, R, **f64))
            if self.w_len != 0.0:
                lm.update(slen=torch.zeros(R, **f64), end_len=torch.zeros(steps, R, **f64))
        if not self.use_ctc:
            st["psi"].zero_()                 # w_ctc = 0 multiplies it: keep it finite
        if not self.use_dec:
            st["dec0"] = torch.zeros(R, V, **f32)
            nch = -(-self.n_vocab // 64)
            ids = torch.arange(nch * 64, dtype=torch.int32)
            ids[ids >= self.n_vocab] = self.blank          # padding ids: blank (psi = LOGZERO)
            st["vchunks"] = ids.view(nch, 1, 64).expand(nch, R, 64).contiguous().to(dev)
            st["psi_c"] = torch.empty(R, 65, **f32)
            st["r_scr"] = torch.empty(R, 64, Tm, 2, **f32)
            st["psi_full"] = torch.empty(R, nch * 64, **f32)
        return st

    def _capture(self, eng, st):
        """two graphs of the generic step (k = 0, 1): capture records, it does not run. The
        capture stream is one long-lived stream per device, and its workspaces (split-K arrival
        counters, which must start at zero, and the dec_attn partials) are created eagerly
        before the capture: a zero-fill recorded inside graph 0 would never run before graph 1's
        first replay."""
        dev = eng.device
        graphs = []
        s = _capture_stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            ops.reserve_stream_workspaces(dev, ops.dec_attn_ws_floats(st["R"], eng.dH, self._cross_group(st["Tm"]), 2))
        for k in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                self._step(eng, st, False, k)
            graphs.append(g)
        torch.cuda.current_stream(dev).wait_stream(s)
        return graphs

    def _ended_hyps(self, st, n, r0, rows):
        """the ended hypotheses recorded in history columns [r0, r0 + rows) over the first n steps,
        as [(column - r0, Hypothesis)] in the reference's order (step, then selection rank), yseq
        rebuilt from the back-pointers (global row indices, all inside the column range: the
        rows of the utterances it holds)"""
        col = slice(r0, r0 + rows)
        bp_prev, bp_tok, flag, esc, edec, ectc = (st[k][:n, col].cpu().numpy() for k in
                                                  ("bp_prev", "bp_tok", "end_flag", "end_score", "end_dec", "end_ctc"))
        extra = {name: st[grp][k][:n, col].cpu().numpy() for name, grp, k in
                 (("hotword", "hw", "end_hw"), ("lm", "lm", "end_lm"), ("length_bonus", "lm", "end_len"))
                 if k in st.get(grp, {})}
        out = []
        for i in range(n):
            for r in np.nonzero(flag[i])[0].tolist():
                toks = [int(bp_tok[i, r])]
                h = int(bp_prev[i, r]) - r0
                for j in range(i - 1, -1, -1):
                    toks.append(int(bp_tok[j, h]))
                    h = int(bp_prev[j, h]) - r0
                yseq = [self.sos] + toks[::-1] + ([self.eos] if flag[i, r] == 2 else [])
                hyp = dict(yseq=yseq, score=float(esc[i, r]), dec=float(edec[i, r]), ctc=float(ectc[i, r]))
                for name, a in extra.items():
                    hyp[name] = float(a[i, r])
                out.append((r, self._make_hyp(hyp, self.use_dec, self.use_ctc)))
        return out

    def _collect(self, st, xs, maxlenratio, minlenratio):
        """ended hypotheses from the device history, per utterance in the reference's order
        (step, then selection rank), yseq rebuilt from the back-pointers"""
        U, R, beam = st["U"], st["R"], self.beam_size
        n = min(int(st["pos"].item()), st["steps"])
        ended = [[] for _ in range(U)]
        for r, hyp in self._ended_hyps(st, n, 0, R):
            ended[r // beam].append(hyp)
        results = []
        for u in range(U):
            nbest = sorted(ended[u], key=lambda h: float(h.score), reverse=True)
            if not nbest and minlenratio >= 0.1:
                nbest = self.forward(xs[u], maxlenratio, max(0.0, minlenratio - 0.1))
            results.append(nbest)
        return results

    # ----------------------------------------------------------------------- streaming
    def stream(self, slots=None, max_frames=375, maxlenratio=0.0, minlenratio=0.0, poll=4, graphs=True):
        """A persistent decode session of `slots` utterance slots x beam rows (see DecodeSession);
        slots=None: min(8, 64 // beam)."""
        return DecodeSession(self, slots, max_frames, maxlenratio, minlenratio, poll, graphs)

    def decode_stream(self, xs, **kw):
        """The n-best lists of the encoded utterances xs in input order, decoded through a session
        (`stream(**kw)`) that refills a slot as soon as its utterance ends. Per utterance the result
        is that of `self(x)`."""
        xs = list(xs)
        with self.stream(**kw) as session:
            return stream_slots.in_input_order(session.run(xs), len(xs))

    @staticmethod
    def _maxlen(T, maxlenratio):
        """steps of an utterance of T frames"""
        return T if maxlenratio == 0 else (-int(maxlenratio) if maxlenratio < 0 else max(1, int(maxlenratio * T)))

    def _session_buffers(self, S, max_frames):
        """what a session owns besides the search state: (engine, device, dtype, D, decoder layers,
        CTC log-probs [S][max_frames][V], per-layer cross K/V [S*max_frames][2D], folded LayerNorms).
        All zero: an empty slot's rows run through every kernel of a step, on finite values.
        With `_session_admit` one of the two places where a session touches the engine: the
        scripted-decoder tests replace both (engine None, no memory, a table decoder), so the real
        admission path is covered by the model tests only (tests/test_gpu_decode_stream.py)."""
        eng = self.e2e.engine()
        if eng.dtype != torch.float32:
            raise NotImplementedError("decode sessions run on the fp32 engine, the evaluation precision of the "
                                      "reference; a bf16 engine decodes with decode_batch")
        dev, D = eng.device, eng.dD
        logp = torch.zeros(S, max_frames, eng.V, device=dev, dtype=torch.float32)
        mem = [torch.zeros(S * max_frames, 2 * D, device=dev, dtype=eng.dtype) for _ in range(eng.dl)]
        fold = self._fold_layernorms(eng) if FOLD_LN and self.use_dec else None
        return eng, dev, eng.dtype, D, eng.dl, logp, mem, fold

    def _session_admit(self, sess, slot, x):
        """utterance x (T, d) into slot `slot` of the session, eagerly on the current stream: the
        launches decode_batch makes per utterance (`_project_memory` over its own T rows), written
        into the slot's regions, and the log-softmax of those T rows. (The second hook the
        scripted-decoder tests replace, see `_session_buffers`.)"""
        eng, st = sess.eng, sess.st
        T = int(x.shape[0])
        xu, cl = sess.xbuf[:T], sess.clbuf[:T]
        ops.cast(x.to(eng.device).reshape(T, eng.dD).contiguous(), xu)
        self._project_memory(eng, xu, cl, st["mem"], slot * st["Tm"])
        ops.log_softmax_rows(cl, eng.V, st["logp"][slot, :T])

    def _new_stream_state(self, device, dtype, S, max_frames, steps, logp, mem, D, layers, end_detect=1, fold=None):
        """the search state of a session: `_new_state` of S utterances of max_frames frames and
        `steps` steps, with every slot empty (done, no live row), the positions per slot (upos)
        and per row (rowpos; also under "pos", which the step's kernels read), and one more
        history row: a done slot stands one past its last record and writes there."""
        st = self._new_state(device, dtype, [max_frames] * S, [steps] * S, logp, mem, D, layers,
                             end_detect=end_detect, fold=fold)
        R = st["R"]
        st["upos"] = torch.zeros(S, device=device, dtype=torch.int32)
        st["rowpos"] = st["pos"] = torch.zeros(R, device=device, dtype=torch.int32)
        st["per_row"] = True
        for k in ("bp_prev", "bp_tok", "end_flag", "end_score", "end_dec", "end_ctc"):
            st[k] = torch.zeros(steps + 1, R, device=device, dtype=st[k].dtype)
        for k in ("ids", "klen_self", "src"):
            st[k].zero_()
        for k in ("psi", "r_new", "psi_c", "r_scr", "psi_full"):
            if k in st:
                st[k].zero_()
        for t in st["r_prev"]:
            t.zero_()
        st["score"].fill_(float("-inf"))
        st["done"].fill_(1)
        st["done"][S] = S
        return st

    def _collect_slot(self, st, slot, n):
        """`_collect` for one slot whose utterance ended after n steps: its history columns"""
        beam = self.beam_size
        ended = [hyp for _, hyp in self._ended_hyps(st, n, slot * beam, beam)]
        return sorted(ended, key=lambda h: float(h.score), reverse=True)

    @staticmethod
    def _make_hyp(hyp, use_dec=True, use_ctc=True):
        """the reference's Hypothesis: scores of the scorers in the search only ("hotword": the
        summed hot-word bonus, only in a search with a phrase list; "lm": the unweighted LM sum and
        "length_bonus": the number of scored tokens, each only at a non-zero weight)"""
        scores = {}
        if use_dec:
            scores["decoder"] = torch.tensor(hyp["dec"], dtype=torch.float32)
        if use_ctc:
            scores["ctc"] = torch.tensor(hyp["ctc"], dtype=torch.float32)
        for k in ("hotword", "length_bonus", "lm"):
            if k in hyp:
                scores[k] = torch.tensor(hyp[k], dtype=torch.float32)
        return Hypothesis(yseq=torch.tensor(hyp["yseq"], dtype=torch.int64),
                          score=torch.tensor(hyp["score"], dtype=torch.float32), scores=scores, states={})


class DecodeSession:
    """A persistent beam-search session over a stream of utterances (continuous batching).

    Geometry fixed at creation: `slots` utterances x beam rows (at most 64 rows, the few-row GEMM's
    limit), `max_frames` memory frames per slot, Lcap = maxlen(max_frames) + 1 positions. The session
    owns one search state, the per-slot memory regions (cross-attention K/V per decoder layer,
    CTC log-probs), the self-attention cache and the two step graphs, captured once. It snapshots
    the folded LayerNorm weights at creation: weights changed afterwards need a new session.

    Every step is one graph replay, a slot's step 0 included: positions are per row on the device,
    so one replay is step 0 of a freshly filled slot and step 200 of its neighbour. An utterance
    is admitted into a free slot eagerly (its memory projections, log-softmax, avsr_beam_slot_reset);
    every `poll` replays the host reads the per-slot done flags (pinned, non-blocking copy and an
    event), collects the n-best of each newly finished slot from its history columns and frees it.
    Per utterance the result equals `bs(x)`: rows never read another slot's state.

    `run(xs)` yields (index, nbest) in completion order; an utterance longer than max_frames is
    decoded alone through `bs(x)` and delivered in its place. A session runs any number of
    streams one after another; `close()` drops graphs and buffers."""

    def __init__(self, bs, slots=None, max_frames=375, maxlenratio=0.0, minlenratio=0.0, poll=4, graphs=True):
        if bs.hotwords is not None:
            raise NotImplementedError("hot words: a decode session does not carry the tree nodes; use decode_batch")
        if bs.lm is not None or bs.w_len != 0.0:
            raise NotImplementedError("LM fusion / length bonus: a decode session does not reset the LM state of a "
                                      "refilled slot; use decode_batch")
        beam = bs.beam_size
        S = stream_slots.default_slots(beam) if slots is None else int(slots)
        stream_slots.check_geometry(S, beam)
        if max_frames < 1 or poll < 1:
            raise ValueError(f"max_frames = {max_frames}, poll = {poll}")
        self.bs, self.S, self.max_frames, self.poll = bs, S, int(max_frames), int(poll)
        self.maxlenratio, self.minlenratio = maxlenratio, minlenratio
        steps = bs._maxlen(self.max_frames, maxlenratio)
        if steps < 1:
            raise ValueError(f"maxlenratio = {maxlenratio}: no step to run")
        self.eng, dev, dtype, D, layers, logp, mem, fold = bs._session_buffers(S, self.max_frames)
        self.device = dev
        if self.eng is not None:
            self.eng.ensure_pe(steps + 1)
            self.xbuf = torch.empty(self.max_frames, D, device=dev, dtype=dtype)
            self.clbuf = torch.zeros(self.max_frames, self.eng.Vp, device=dev, dtype=dtype)
        self.st = bs._new_stream_state(dev, dtype, S, self.max_frames, steps, logp, mem, D, layers,
                                       end_detect=int(maxlenratio == 0.0), fold=fold)
        self.book = None
        self.k = 0                              # ping-pong buffer the next step reads
        self.replays = 0                        # steps run so far, over all streams
        self._host = torch.empty(2 * S + 1, dtype=torch.int32).pin_memory()    # done[S + 1], upos[S]
        self._event = torch.cuda.Event()
        self.graphs = bs._capture(self.eng, self.st) if graphs else None
        self._ws = None
        if graphs:
            # what the graphs point into besides the session's own state, kept alive with them: the
            # capture stream's workspaces and the engine's positional-encoding table (a later, longer
            # search makes the engine allocate a new table; the graphs go on reading this one, whose
            # rows are the same values)
            key = (ops._norm_dev(dev), _capture_stream(dev).cuda_stream)
            self._ws = (ops._SKINNY_WS.get(key), ops._DA_WS.get(key), None if self.eng is None else self.eng._pe)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.graphs = self.st = self._ws = None
        self.xbuf = self.clbuf = None

    def _step(self):
        if self.graphs is not None:
            self.graphs[self.k].replay()
        else:
            self.bs._step(self.eng, self.st, False, self.k)
        self.k ^= 1
        self.replays += 1

    def _admit(self, slot, x):
        bs, st = self.bs, self.st
        T = int(x.shape[0])
        bs._session_admit(self, slot, x)
        ops.beam_slot_reset(U=self.S, beam=bs.beam_size, Lmax=st["Lmax"], slot=slot, sos=bs.sos,
                            maxlen=bs._maxlen(T, self.maxlenratio), tlen=T, upos=st["upos"], rowpos=st["rowpos"],
                            done=st["done"], tok=st["tok"], score=st["score"], sdec=st["sdec"], sctc=st["sctc"],
                            s_prev=st["s_prev"], best_len=st["best_len"], best_end=st["best_end"],
                            maxlen_arr=st["maxlen"], tlen_arr=st["tlen"], klen_mem=st["klen_mem"])

    def _poll(self):
        """(done per slot, position per slot) as of the steps issued so far"""
        S, st = self.S, self.st
        self._host[:S + 1].copy_(st["done"], non_blocking=True)
        self._host[S + 1:].copy_(st["upos"], non_blocking=True)
        self._event.record()
        self._event.synchronize()
        h = self._host.tolist()
        return h[:S], h[S + 1:]

    def run(self, xs):
        """generator of (index, nbest) in completion order for the encoded utterances xs (an
        iterable, consumed as slots become free)"""
        if self.st is None:
            raise RuntimeError("the session is closed")
        bs = self.bs
        book = self.book = stream_slots.SlotBook(self.S, bs.beam_size, self.max_frames)   # (kept for inspection)
        inputs = enumerate(xs)
        held, limit, ran = {}, {}, {}           # per busy slot: its input, its maxlen, its steps so far
        budget, start, since, more = 0, self.replays, 0, True
        while True:
            while more and book.free_slot() is not None:
                nxt = next(inputs, None)
                if nxt is None:
                    more = False
                    break
                i, x = nxt
                if not book.fits(int(x.shape[0])):      # oversize: the one-utterance search, in its place
                    yield book.bypass(i), bs.forward(x, self.maxlenratio, self.minlenratio)
                    continue
                slot = book.admit(i, int(x.shape[0]))
                self._admit(slot, x)
                held[slot], limit[slot], ran[slot] = x, bs._maxlen(int(x.shape[0]), self.maxlenratio), 0
                budget += limit[slot]
            busy = book.busy()
            if not busy:
                break
            if self.replays - start >= budget + self.poll:
                raise RuntimeError(f"decode session: {self.replays - start} steps for a budget of {budget}")
            self._step()
            since += 1
            for slot in busy:
                ran[slot] += 1
            # nothing can have ended before its first `poll`-th step unless a slot is at its limit
            if since < self.poll and not any(ran[s] >= limit[s] for s in busy):
                continue
            since = 0
            done, upos = self._poll()
            for slot in sorted(busy):
                if not done[slot]:
                    if ran[slot] >= limit[slot]:
                        raise RuntimeError(f"decode session: slot {slot} not done after its {limit[slot]} steps")
                    continue
                nbest = bs._collect_slot(self.st, slot, min(upos[slot], limit[slot]))
                x = held.pop(slot)
                if not nbest and self.minlenratio >= 0.1:
                    nbest = bs.forward(x, self.maxlenratio, max(0.0, self.minlenratio - 0.1))
                yield book.finish(slot), nbest


def get_beam_search_decoder(model, token_list, ctc_weight=0.1, beam_size=3, hotwords=None, hotword_bonus=None,
                            lm=None, lm_weight=0.0, length_bonus=0.0):
    """src/avhubert_avsr/avhubert_avsr_model.py:12-36 — `model` is the E2E (`AVHubertAVSR.avsr`).
    hotwords (token-id lists) and hotword_bonus: `set_hotwords` on the result; lm (an NgramLM),
    lm_weight and length_bonus: `set_lm` (the two scorer slots the reference hard-wires to 0)."""
    weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": 0.0, "length_bonus": 0.0}
    bs = BatchBeamSearch(model, beam_size=beam_size, vocab_size=len(token_list), weights=weights, sos=model.sos,
                         eos=model.eos, token_list=token_list,
                         pre_beam_score_key=None if ctc_weight == 1.0 else "decoder")
    bs.set_hotwords(hotwords, hotword_bonus)
    bs.set_lm(lm, lm_weight, length_bonus)
    return bs

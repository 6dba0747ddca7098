"""How sure the model is of each token / word: confidences of hypotheses on the HIP engine.

For a hypothesis y = y_1..y_L the CTC head gives an exact answer to "this token, against every
alternative for its slot": with sub[l][v] = log p_ctc(y with y_l replaced by v | x) and
del[l] = log p_ctc(y without y_l | x) (avsr_ctc_neighbors, include/avsr_hip.h: all L * (V - 1) + L
one-edit neighbours in one launch),

    Z_l = LSE(sub[l][v] over v != blank, eos; del[l])       conf_ctc(l) = exp(sub[l][y_l] - Z_l)

is the posterior of y_l among the one-edit outcomes of slot l; an alternative v has
exp(sub[l][v] - Z_l), the deletion exp(del[l] - Z_l). Insertions are not considered. The decoder
term is conf_dec(l) = p_dec(y_l | sos, y_1..y_{l-1}, x) of one teacher-forced pass (the code path of
the two-pass decoder's rescoring), and the joint value combines them as the searches combine their
scorers:

    conf(l) = exp((1 - w) * log conf_dec(l) + w * log conf_ctc(l)),   w = ctc_weight

(w = 0 or 1: one term alone, the other is not computed). It needs no training and no data; ITS
CALIBRATION IS UNMEASURED (no checkpoint or data here): read it as a ranking of tokens, not as
the probability that a token is right.

    conf = confidence_batch(model.avsr, [enc_u for ...], [hyp.yseq for ...], ctc_weight=0.1)
    words = word_confidences(conf[0].tokens, token_list)      # zips with align.word_times
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .align import strip_sos_eos, word_groups
from .rescore import ctc_feasible, ctc_logits, decoder_token_logp

# ctc / decoder / joint in (0, 1] (None: that scorer is not in use); alternatives: [(token id, or
# None for the deletion, posterior)] best first
TokenConfidence = namedtuple("TokenConfidence", ["token", "ctc", "decoder", "joint", "alternatives"])
# eos: the decoder's probability of ending after y (None at ctc_weight 1); utterance: geometric
# mean of the joint values; base: log p_ctc(y | x) (None at ctc_weight 0)
Confidence = namedtuple("Confidence", ["tokens", "eos", "utterance", "base"])

MAX_ALTERNATIVES = 16       # avsr_row_topk's K


def joint_confidence(dec_logp, ctc_logp, w):
    """exp((1 - w) * log conf_dec + w * log conf_ctc); one term alone where the other is None"""
    if dec_logp is None:
        return math.exp(ctc_logp)
    if ctc_logp is None:
        return math.exp(dec_logp)
    return math.exp((1.0 - w) * dec_logp + w * ctc_logp)


def rank_alternatives(cands, k):
    """the k best of [(token or None for the deletion, score)]: score descending, ties to the
    lower id, the deletion last among equals; outcomes without a CTC path (-inf) are left out"""
    live = [(tok, s) for tok, s in cands if s > -math.inf]
    live.sort(key=lambda c: (-c[1], c[0] is None, -1 if c[0] is None else c[0]))
    return live[:k]


@torch.no_grad()
def confidence_batch(e2e, xs, yseqs, ctc_weight=0.1, alternatives=0):
    """Confidences of U hypotheses: xs = list of encoded utterances (T_u, D), yseqs = list of
    token-id sequences (a leading sos / trailing eos, as in Hypothesis.yseq, is stripped) from any
    search or a human transcript. Returns per utterance Confidence(tokens, eos, utterance, base),
    or None where y has no CTC path (fewer frames than labels + adjacent repeats).

    The CTC logits are computed per utterance (rescore.ctc_logits: the result of an utterance does
    not depend on the batch); then ONE avsr_ctc_neighbors launch for the padded batch, for
    alternatives > 0 one avsr_row_topk over its rows, one teacher-forced decoder pass per
    utterance, and ONE host read of everything."""
    if len(xs) != len(yseqs):
        raise ValueError(f"{len(xs)} utterances but {len(yseqs)} token sequences")
    w = float(ctc_weight)
    if not 0.0 <= w <= 1.0:
        raise ValueError(f"ctc_weight {ctc_weight} outside [0, 1]")
    K = int(alternatives)
    if not 0 <= K <= MAX_ALTERNATIVES or K != alternatives:
        raise ValueError(f"alternatives {alternatives} outside [0, {MAX_ALTERNATIVES}]")
    U = len(xs)
    if U == 0:
        return []
    eng = e2e.engine()
    dev, V, blank, sos, eos = eng.device, eng.V, e2e.blank, e2e.sos, e2e.eos
    ys = [strip_sos_eos(y, sos, eos) for y in yseqs]
    for u, y in enumerate(ys):
        if any(t < 0 or t >= V for t in y):
            raise ValueError(f"utterance {u}: token id outside [0, {V})")
        if any(t == blank or t == eos for t in y):
            raise ValueError(f"utterance {u}: blank / eos inside the token sequence")
        if len(y) > ops.CTC_BEAM_LCAP:
            raise ValueError(f"utterance {u}: {len(y)} tokens, avsr_ctc_neighbors takes at most {ops.CTC_BEAM_LCAP}")
    use_dec, use_ctc = w != 1.0, w != 0.0
    xp, cl, Ts, Tm = ctc_logits(eng, xs)
    feas = [ctc_feasible(Ts[u], ys[u]) and Ts[u] > 0 for u in range(U)]
    Lmax = max(1, max(len(y) for y in ys))
    parts = []
    if use_ctc:
        lab = torch.full((U, Lmax), -1, dtype=torch.int32)
        for u, y in enumerate(ys):
            lab[u, :len(y)] = torch.tensor(y, dtype=torch.int32)
        lab = lab.to(dev)
        lse = torch.empty(U * Tm, device=dev, dtype=torch.float32)
        ops.row_lse(cl, V, lse)
        lz = torch.empty(U, Lmax, device=dev, dtype=torch.float32)
        sub, dele, base, kfeas = ops.ctc_neighbors(
            cl, U, Tm, V, lab, torch.tensor([len(y) for y in ys], dtype=torch.int32).to(dev),
            torch.tensor(Ts, dtype=torch.int32).to(dev), lse, blank=blank, eos=eos, lz=lz)
        own_idx = lab.clamp(min=0).long().unsqueeze(-1)
        own = sub.gather(2, own_idx).squeeze(-1)                       # sub[u][l][y_l]
        parts += [base, kfeas.float(), dele.reshape(-1), lz.reshape(-1), own.reshape(-1)]
        if K:
            # the K best OTHER tokens of every slot: the row with its own token taken out
            others = sub.scatter(2, own_idx, float("-inf"))
            ids = torch.empty(U * Lmax, K, device=dev, dtype=torch.int32)
            ops.row_topk(others.view(U * Lmax, -1), V, K, ids)
            ids = ids.view(U, Lmax, K).clamp(0, V - 1)                  # fewer than K columns: filler ids
            parts += [others.gather(2, ids.long()).reshape(-1), ids.float().reshape(-1)]   # ids < 2^24: exact
    if use_dec:
        dec_off = {}
        for u in range(U):
            if feas[u]:
                dec_off[u] = sum(int(p.numel()) for p in parts)
                parts.append(decoder_token_logp(eng, xp[u, :Ts[u]], [ys[u]], sos, eos))
    host = torch.cat(parts).cpu().numpy().astype(np.float64) if parts else np.zeros(0)
    if use_ctc:
        o = 0
        h_base, h_feas = host[o:o + U], host[o + U:o + 2 * U]
        o += 2 * U
        h_del, h_lz, h_own = (host[o + i * U * Lmax:o + (i + 1) * U * Lmax].reshape(U, Lmax) for i in range(3))
        o += 3 * U * Lmax
        if K:
            h_tv = host[o:o + U * Lmax * K].reshape(U, Lmax, K)
            h_ti = host[o + U * Lmax * K:o + 2 * U * Lmax * K].reshape(U, Lmax, K).astype(np.int64)
        feas = [bool(f) and h for f, h in zip(h_feas, feas)]           # the kernel's verdict: the same rule
    out = []
    for u, y in enumerate(ys):
        if not feas[u]:
            out.append(None)
            continue
        dec = host[dec_off[u]:dec_off[u] + len(y) + 1] if use_dec else None
        toks, logs = [], []
        for l, tok in enumerate(y):
            c_log, alts = None, []
            if use_ctc:
                z = h_base[u] + h_lz[u, l]                              # Z_l
                c_log = min(0.0, h_own[u, l] - h_base[u] - h_lz[u, l])  # <= 0 up to fp32 rounding of lz
                if K:
                    cands = [(int(h_ti[u, l, r]), float(h_tv[u, l, r])) for r in range(K)] + [(None, float(h_del[u, l]))]
                    alts = [(t, math.exp(min(0.0, s - z))) for t, s in rank_alternatives(cands, K)]
            d_log = float(dec[l]) if use_dec else None
            j = joint_confidence(d_log, c_log, w)
            logs.append(d_log if c_log is None else (c_log if d_log is None else (1.0 - w) * d_log + w * c_log))
            toks.append(TokenConfidence(tok, None if c_log is None else math.exp(c_log),
                                        None if d_log is None else math.exp(d_log), j, alts))
        out.append(Confidence(toks, math.exp(float(dec[len(y)])) if use_dec else None,
                              math.exp(sum(logs) / len(logs)) if logs else 1.0,
                              float(h_base[u]) if use_ctc else None))
    return out


def word_confidences(tokens, token_list, agg="min", space="▁"):
    """[(word, confidence)] from the TokenConfidences of a hypothesis: align.word_times' word
    segmentation (the two lists zip), `agg` of the joint values of a word's pieces -- "min" (a word
    is as sure as its least sure piece), "prod" or "mean"."""
    if agg not in ("min", "prod", "mean"):
        raise ValueError(f"agg {agg!r}: one of 'min', 'prod', 'mean'")
    out = []
    for word, idx in word_groups([t.token for t in tokens], token_list, space):
        vals = [float(tokens[i].joint) for i in idx]
        c = min(vals) if agg == "min" else (math.prod(vals) if agg == "prod" else sum(vals) / len(vals))
        out.append((word, c))
    return out

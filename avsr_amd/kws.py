"""Is a phrase said in an utterance, and when: keyword spotting on the CTC posteriors of the HIP
engine, without decoding.

For a keyword y = y_1..y_L (token ids) avsr_ctc_kws (include/avsr_hip.h) finds the span of frames
[start, end) and the CTC path of y over exactly that span which maximise

    score = sum over the span of  log p_ctc(path_t | x) - log p_ctc(best token of frame t | x)

-- the CTC Viterbi of y with a free start and a free end, against a filler that reads every frame
as its best token. score <= 0, and 0 means the keyword IS the greedy reading of its span. One
launch scores K keywords x U utterances (one wavefront per pair); nothing is decoded, so a phrase
that a beam search would have pruned is still found, and a keyword list costs far less than a
search.

    hits = spot_batch(model.avsr, [enc_u for ...], hotwords.encode(["hello world"], tokenize),
                      threshold=-2.0)
    for h in hits[0]:
        print(h.keyword, hit_times(h, frame_rate=cfg.label_rate), h.avg)

`avg` = score / (end - start) is what a threshold applies to. WHAT THRESHOLD SEPARATES HITS FROM
FALSE ALARMS, AND THE DETECTION ACCURACY, ARE UNMEASURED (no checkpoint or data here): without a
threshold every keyword that fits into the utterance comes back with its best span.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .rescore import ctc_logits

# keyword: index into the keyword list; frames [start, end); score <= 0; avg = score / (end - start)
KeywordHit = namedtuple("KeywordHit", ["keyword", "start", "end", "score", "avg"])

MAX_TOKENS = ops.CTC_KWS_LMAX


def check_keywords(keywords, V, blank, eos):
    """keywords as lists of ints, or ValueError: an empty list, an empty keyword, a blank / eos /
    negative / >= V id, more than MAX_TOKENS tokens. (Bad input is refused here, on the host; the
    kernel's -inf is for keywords that do not fit into an utterance.)"""
    kws = [[int(t) for t in y] for y in keywords]
    if not kws:
        raise ValueError("no keywords")
    for k, y in enumerate(kws):
        if not y:
            raise ValueError(f"keyword {k} is empty")
        if len(y) > MAX_TOKENS:
            raise ValueError(f"keyword {k}: {len(y)} tokens, avsr_ctc_kws takes at most {MAX_TOKENS}")
        if any(t < 0 or t >= V for t in y):
            raise ValueError(f"keyword {k}: token id outside [0, {V})")
        if any(t == blank or t == eos for t in y):
            raise ValueError(f"keyword {k}: blank / eos inside the keyword")
    return kws


def _hit(keyword, score, start, end):
    score, start, end = float(score), int(start), int(end)
    return KeywordHit(keyword, start, end, score, score / (end - start))


def _keeps(avg, threshold):
    return threshold is None or avg >= threshold


def select_occurrences(trace, tstart, threshold=None, keyword=0):
    """Non-overlapping occurrences of one keyword in one utterance from the kernel's traces
    (trace[t], tstart[t]: score and start of the best occurrence ending at frame t). Candidates
    are all t with a finite trace, (score = trace[t], start = tstart[t], end = t + 1); those with
    avg >= threshold (None: all) are taken by score descending, the later end first on ties, and
    a candidate is accepted when its span overlaps no accepted one. Returns the accepted
    KeywordHits sorted by start; the first one accepted is the kernel's best occurrence."""
    trace = np.asarray(trace, dtype=np.float64)
    tstart = np.asarray(tstart)
    cands = [_hit(keyword, trace[t], tstart[t], t + 1) for t in range(len(trace)) if math.isfinite(trace[t])]
    cands = [c for c in cands if _keeps(c.avg, threshold)]
    cands.sort(key=lambda c: (-c.score, -c.end))
    taken = []
    for c in cands:
        if all(c.end <= a.start or a.end <= c.start for a in taken):
            taken.append(c)
    return sorted(taken, key=lambda c: (c.start, c.end))


def hit_times(hit, frame_rate=25.0):
    """(start_s, end_s) of a KeywordHit: frames / frame_rate (the config's label_rate)"""
    return hit.start / frame_rate, hit.end / frame_rate


def _spot_logits(eng, cl, Ts, Tm, kws, blank, threshold, occurrences):
    """log-softmax + argmax of every row of the CTC logits cl (U*Tm, Vp), ONE avsr_ctc_kws launch,
    one host read -> per utterance the KeywordHits sorted by start"""
    U, K, dev, V = len(Ts), len(kws), eng.device, eng.V
    logp = torch.empty(U, Tm, V, device=dev, dtype=torch.float32)
    top = torch.empty(U, Tm, device=dev, dtype=torch.int32)
    ops.log_softmax_topk(cl, V, logp.view(U * Tm, V), 1, top.view(U * Tm, 1))
    Lmax = max(len(y) for y in kws)
    lab = torch.full((K, Lmax), -1, dtype=torch.int32)
    for k, y in enumerate(kws):
        lab[k, :len(y)] = torch.tensor(y, dtype=torch.int32)
    out = ops.ctc_kws(logp, torch.tensor(Ts, dtype=torch.int32).to(dev), top, lab.to(dev),
                      torch.tensor([len(y) for y in kws], dtype=torch.int32).to(dev), blank=blank, trace=occurrences)
    # one read: the int32 outputs are frame indices, exact in fp32
    host = torch.cat([t.reshape(-1).float() for t in out]).cpu().numpy()
    n = U * K
    score, start, end = (host[i * n:(i + 1) * n].reshape(U, K) for i in range(3))
    if occurrences:
        trace, tstart = (host[3 * n + i * n * Tm:3 * n + (i + 1) * n * Tm].reshape(U, K, Tm) for i in range(2))
    hits = []
    for u in range(U):
        hu = []
        for k in range(K):
            if not math.isfinite(score[u, k]):
                continue
            if occurrences:
                hu += select_occurrences(trace[u, k, :Ts[u]], tstart[u, k, :Ts[u]].astype(np.int64), threshold, k)
            else:
                h = _hit(k, score[u, k], start[u, k], end[u, k])
                if _keeps(h.avg, threshold):
                    hu.append(h)
        hits.append(sorted(hu, key=lambda h: (h.start, h.end, h.keyword)))
    return hits


@torch.no_grad()
def spot_batch(e2e, xs, keywords, threshold=None, occurrences=False):
    """Keyword spotting over U utterances: xs = list of encoded utterances (T_u, D), keywords =
    list of token-id lists (texts: hotwords.encode). Returns per utterance a list of KeywordHits
    sorted by start: with occurrences=False the best occurrence of every keyword that has a path
    (at least as many frames as tokens + adjacent repeats) and whose avg >= threshold (None: no
    threshold); with occurrences=True every non-overlapping occurrence (select_occurrences).

    The CTC logits are computed per utterance (rescore.ctc_logits: the result of an utterance does
    not depend on the batch); then ONE log-softmax + argmax over all rows, ONE avsr_ctc_kws launch
    for all keywords x utterances, and ONE host read."""
    eng = e2e.engine()
    kws = check_keywords(keywords, eng.V, e2e.blank, e2e.eos)
    if len(xs) == 0:
        return []
    _, cl, Ts, Tm = ctc_logits(eng, xs)
    return _spot_logits(eng, cl, Ts, Tm, kws, e2e.blank, threshold, occurrences)

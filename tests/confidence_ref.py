"""Reference of the one-edit-neighbour confidences (include/avsr_hip.h avsr_ctc_neighbors,
avsr_amd/confidence.py), in fp64 on the CPU. A helper, not a test.

The oracle is NOT the shared alpha / beta derivation the kernel uses: every neighbour's
likelihood is torch.nn.functional.ctc_loss on that neighbour's explicit label sequence."""
import math

import torch
import torch.nn.functional as F

NEG_INF = float("-inf")


def _ctc_logp(logp, targets, n, blank):
    """log p_ctc of each row of targets (N, L) int64 over the first n frames of logp (T, V) fp64;
    -inf where no path exists"""
    N, L = targets.shape
    lp = logp[:n].unsqueeze(1).expand(n, N, logp.shape[1])
    if L == 0:
        return lp[:, 0, blank].sum().expand(N).clone()
    nll = F.ctc_loss(lp, targets, torch.full((N,), n, dtype=torch.long), torch.full((N,), L, dtype=torch.long),
                     blank=blank, reduction="none", zero_infinity=False)
    out = -nll
    out[torch.isinf(nll)] = NEG_INF
    return out


def neighbors(logp, y, n, blank=0, eos=-1, slots=None, cols=None):
    """sub (L, V), del (L,), base of labels y over the first n frames of log-probs logp (T, V),
    all fp64: sub[l][v] = log p_ctc(y with y_l := v), -inf at v = blank / eos and where the
    neighbour has no path; del[l] = log p_ctc(y without y_l); base = log p_ctc(y). `slots` /
    `cols` restrict sub to those rows / columns (the others stay NaN: not computed)."""
    logp = logp.double()
    V, L = logp.shape[1], len(y)
    yt = torch.tensor(list(y), dtype=torch.long)
    base = float(_ctc_logp(logp, yt.view(1, L), n, blank)[0])
    sub = torch.full((L, V), float("nan"), dtype=torch.float64)
    dele = torch.full((L,), NEG_INF, dtype=torch.float64)
    vs = torch.arange(V) if cols is None else torch.tensor(sorted(set(int(c) for c in cols)), dtype=torch.long)
    ok = (vs != blank) & (vs != eos)
    for l in range(L):
        rest = torch.cat([yt[:l], yt[l + 1:]])
        dele[l] = _ctc_logp(logp, rest.view(1, L - 1), n, blank)[0]
        if slots is not None and l not in slots:
            continue
        tg = yt.repeat(int(ok.sum()), 1)
        tg[:, l] = vs[ok]
        row = torch.full((len(vs),), NEG_INF, dtype=torch.float64)
        row[ok] = _ctc_logp(logp, tg, n, blank)
        sub[l, vs] = row
    return sub, dele, base


def posteriors(sub, dele, y, k=0, blank=0, eos=-1):
    """per slot (conf_ctc, [(token or None for the deletion, posterior)] the k best other outcomes):
    Z_l = LSE(sub[l][allowed v], del[l]) in fp64; alternatives best first, ties to the lower id,
    the deletion last among equals, outcomes of posterior 0 (no CTC path) left out"""
    out = []
    for l, tok in enumerate(y):
        row = sub[l].double().clone()
        row[blank] = NEG_INF
        if eos >= 0:
            row[eos] = NEG_INF
        z = torch.logsumexp(torch.cat([row, dele[l].double().view(1)]), 0).item()
        cands = [(v, float(row[v])) for v in range(row.numel()) if v != tok and float(row[v]) > NEG_INF]
        if float(dele[l]) > NEG_INF:
            cands.append((None, float(dele[l])))
        cands.sort(key=lambda c: (-c[1], c[0] is None, -1 if c[0] is None else c[0]))
        out.append((math.exp(float(row[tok]) - z), [(t, math.exp(s - z)) for t, s in cands[:k]]))
    return out


def word_agg(values, agg):
    """the three word aggregations over the joint confidences of a word's pieces"""
    if agg == "min":
        return min(values)
    if agg == "prod":
        r = 1.0
        for v in values:
            r *= v
        return r
    if agg == "mean":
        return sum(values) / len(values)
    raise ValueError(agg)

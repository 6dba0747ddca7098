"""CTC prefix beam search restated in fp64 with a Python dict keyed by token tuples: the yardstick
of the avsr_ctc_beam kernel tests. Uses none of the project's code.

Semantics (include/avsr_hip.h avsr_ctc_beam): start with the empty prefix at pb = 0, pnb = -inf;
per frame, for each prefix l of the beam with tot = logaddexp(pb, pnb):
    next[l].pb (+)= tot + logp[t][blank]
    for each candidate c of the frame (blank and eos entries skipped), p = logp[t][c]:
        c == last(l):  next[l].pnb (+)= pnb + p  and  next[l + c].pnb (+)= pb + p
        otherwise:     next[l + c].pnb (+)= tot + p          (no extension beyond Lcap tokens)
    keep the N entries with the largest logaddexp(pb, pnb); ties: an entry already in the beam
    ranks by its own place there, a new one by (parent rank, candidate column) after it.

Each case also gets its MARGIN: the smallest gap, in units of 2 * tol, between the N-th and
(N + 1)-th entry at every frame's cut and between successive entries after the last frame, with

    tol(s) = T * 2^-21 * |s| + 1e-5.

Derivation (not a measurement): per frame a prefix score passes through at most four fp32
roundings at magnitude |s| (tot, + p, one or two merges), each <= 2^-24 |s|: T * 2^-22 |s| after
T frames, doubled; every expf / log1pf of an argument <= log 2 adds about 1e-7 absolute, which
the 1e-5 term covers. A case whose margin is below 1 could legitimately come out in another
order in fp32 and is skipped — decided from this fp64 restatement alone. At most MAX_SKIP_SHARE
of the cases of a configuration may be skipped.
"""
import math

import numpy as np

NEG_INF = float("-inf")
MAX_SKIP_SHARE = 0.10
V = 32
BLANK, EOS = 0, V - 1
FIRST_SEED = 2001
SEEDS_PER_CONFIG = 20
# (N, C) per input kind; randn3 at (16, 16) skips too often (near-ties among 16 flat entries)
CONFIGS = {
    "randn3": [(1, 4), (3, 4), (4, 8), (8, 8), (10, 16)],
    "peaked": [(1, 4), (3, 4), (4, 8), (8, 8), (10, 16), (16, 16)],
}
# (kind, N, C, T, seed): cases found by scanning seeds of the restatement for the two rare events,
# a merge with a re-created prefix ('three') and the empty prefix surviving to the end ('peaked')
EXTRA = [("three", 3, 2, 5, 2002), ("three", 3, 2, 5, 2532), ("three", 4, 3, 6, 2035), ("three", 4, 3, 6, 2128),
         ("peaked", 2, 2, None, 2198), ("peaked", 2, 2, None, 2418), ("peaked", 3, 4, None, 2418),
         ("peaked", 3, 4, None, 2474)]
EVENTS = ("repeat_split", "merge_in_beam", "merge_recreated", "empty_survives", "cand_blank", "cand_eos")


def lae(a, b):
    m = max(a, b)
    if m == NEG_INF:
        return NEG_INF
    return m + math.log1p(math.exp(min(a, b) - m))


def tol(s, T):
    return T * 2.0 ** -21 * abs(s) + 1e-5


def topk_ids(logp, C):
    """per frame the C largest columns, value descending then index ascending (avsr_row_topk)"""
    out = np.empty((logp.shape[0], C), dtype=np.int32)
    idx = np.arange(logp.shape[1])
    for t in range(logp.shape[0]):
        out[t] = np.lexsort((idx, -logp[t].astype(np.float64)))[:C]
    return out


def make_case(seed, kind, T=None):
    """(logp (T, V) float32, T): 'randn3' = log_softmax(3 * randn); 'peaked' = log_softmax(randn
    with +6 on one token per frame, blank with probability 1/2); 'three' = 0.3 * randn with
    +U(2, 7) on blank and tokens 1, 2. T drawn from 6..20 unless given."""
    rng = np.random.default_rng(seed)
    drawn = int(rng.integers(6, 21))
    T = drawn if T is None else T
    if kind == "randn3":
        x = 3.0 * rng.standard_normal((T, V))
    elif kind == "peaked":
        x = rng.standard_normal((T, V))
        for t in range(T):
            tok = BLANK if rng.random() < 0.5 else int(rng.integers(1, V))
            x[t, tok] += 6.0
    elif kind == "three":                    # blank and two tokens carry nearly all the mass: dense merging
        x = 0.3 * rng.standard_normal((T, V))
        x[:, [BLANK, 1, 2]] += rng.uniform(2.0, 7.0, size=(T, 3))
    else:
        raise ValueError(kind)
    x = x - x.max(axis=1, keepdims=True)
    logp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    return logp.astype(np.float32)


def search(logp, cand, N, blank=BLANK, eos=EOS, Lcap=None):
    """-> dict(hyps=[(tokens tuple, score)] best first, margin=float, events=set of EVENTS)"""
    T = logp.shape[0]
    Lcap = T if Lcap is None else Lcap
    lp = logp.astype(np.float64)
    beam = [((), 0.0, NEG_INF)]
    birth = {(): -1}                       # frame at which a beam entry (re-)entered the beam
    margin = float("inf")
    events = set()
    for t in range(T):
        nxt, order = {}, {}
        rank_of = {l: i for i, (l, _, _) in enumerate(beam)}

        def acc(key, which, v, okey):
            e = nxt.setdefault(key, [NEG_INF, NEG_INF])
            e[which] = lae(e[which], v)
            okey = (rank_of[key], 0, 0) if key in rank_of else okey
            order[key] = min(order.get(key, okey), okey)

        for i, (l, pb, pnb) in enumerate(beam):
            tot = lae(pb, pnb)
            acc(l, 0, tot + lp[t, blank], (i, 0, 0))
            for j, c in enumerate(int(c) for c in cand[t]):
                if c == blank or c == eos:
                    events.add("cand_blank" if c == blank else "cand_eos")
                    continue
                p = lp[t, c]
                repeat = bool(l) and c == l[-1]
                if repeat:
                    acc(l, 1, pnb + p, (i, 0, 0))
                if len(l) + 1 > Lcap:
                    continue
                nl = l + (c,)
                if repeat:
                    events.add("repeat_split")
                if nl in rank_of:
                    events.add("merge_in_beam")
                    if birth[l] > birth[nl]:
                        events.add("merge_recreated")
                acc(nl, 1, (pb if repeat else tot) + p, (i, 1, j))
        items = sorted(((lae(e[0], e[1]), order[k], k, e) for k, e in nxt.items()), key=lambda x: (-x[0], x[1]))
        if len(items) > N and items[N][0] > NEG_INF:
            a, b = items[N - 1][0], items[N][0]
            margin = min(margin, (a - b) / (2 * tol(max(abs(a), abs(b)), T)))
        items = items[:N]
        birth = {k: (birth[k] if k in rank_of else t) for _, _, k, _ in items}
        beam = [(k, e[0], e[1]) for _, _, k, e in items]
    hyps = [(l, lae(pb, pnb)) for l, pb, pnb in beam] if T > 0 else []
    for (_, a), (_, b) in zip(hyps, hyps[1:]):
        if b > NEG_INF:
            margin = min(margin, (a - b) / (2 * tol(max(abs(a), abs(b)), T)))
    if any(l == () for l, _ in hyps):
        events.add("empty_survives")
    return dict(hyps=hyps, margin=margin, events=events)


_CASES = {}


def case(kind, N, C, seed, T=None):
    """the shared, cached case (logp, cand, reference) of a configuration and seed"""
    key = (kind, N, C, seed, T)
    if key not in _CASES:
        logp = make_case(seed, kind, T)
        cand = topk_ids(logp, C)
        _CASES[key] = dict(logp=logp, cand=cand, T=logp.shape[0], N=N, C=C, ref=search(logp, cand, N))
    return _CASES[key]


def config_cases(kind, N, C):
    return [case(kind, N, C, s) for s in range(FIRST_SEED, FIRST_SEED + SEEDS_PER_CONFIG)]


def extra_cases():
    return [case(kind, N, C, seed, T) for kind, N, C, T, seed in EXTRA]

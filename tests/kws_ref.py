"""Plain numpy free-start / free-end CTC Viterbi with exactly the recursion, roundings and tie
order of avsr_ctc_kws (include/avsr_hip.h), vectorised over the states. A helper, not a test: in
float32 it reproduces the kernel bit for bit; `dtype=np.float64` gives the fp64 DP of the same
log-probs. brute_force() is the definition it is checked against: the pinned CTC Viterbi of the
keyword over every span [s, e), maximised over the spans.

  ext = y1, blank, y2, blank, ..., yL                           S = 2L - 1 states
  f(t) = logp[t][top[t]] (0 without top);  r(t, s) = logp[t][ext_s] - f(t)
  before frame 0 every state is -inf with start -1; per frame, in the order stay, s-1, s-2, enter,
  every comparison strict:
      m, b = d[s], st[s];  d[s-1] > m: take it;  skip(s) and d[s-2] > m: take it;
      s == 0 and 0 > m: m, b = 0, t
      d[s] = m + r(t, s);  st[s] = b, -1 where d[s] is -inf
  score = max_t d[t][S-1], the LAST such t on ties;  end = t + 1;  start = st[t][S-1]
"""
import numpy as np


def _feasible(y, n, Lmax, V, blank):
    L = len(y)
    if n <= 0 or L < 1 or (Lmax is not None and L > Lmax):
        return False
    if any(t < 0 or t >= V or t == blank for t in y):
        return False
    return n >= L + sum(a == b for a, b in zip(y, y[1:]))


def spot(logp, y, n, top=None, blank=0, V=None, Lmax=None, Tm=None, dtype=np.float32):
    """one (utterance, keyword) pair: logp (>= n, >= V) log-probs, y the keyword's ids, n frames,
    top (>= n,) the row argmax or None -> (score, start, end, trace (Tm,), tstart (Tm,) int32);
    no path: (-inf, -1, -1, all -inf, all -1). Tm defaults to max(n, 0); rows >= n are not read."""
    y = [int(t) for t in y]
    logp = np.asarray(logp)
    V = logp.shape[1] if V is None else V
    Tm = max(n, 0) if Tm is None else Tm
    n = min(n, Tm)
    ninf = dtype(-np.inf)
    trace = np.full(Tm, ninf, dtype=dtype)
    tstart = np.full(Tm, -1, dtype=np.int32)
    if not _feasible(y, n, Lmax, V, blank):
        return ninf, -1, -1, trace, tstart
    S = 2 * len(y) - 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[0::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    lp = logp[:n]
    e = lp[:, ext].astype(dtype)
    f = np.zeros(n, dtype=dtype) if top is None else lp[np.arange(n), np.asarray(top)[:n]].astype(dtype)
    r = e - f[:, None]
    assert r.dtype == dtype
    d = np.full(S, ninf, dtype=dtype)
    st = np.full(S, -1, dtype=np.int32)
    best, bt, bs = ninf, -1, -1
    for t in range(n):
        d1 = np.concatenate([[ninf], d[:-1]]).astype(dtype)
        s1 = np.concatenate([[-1], st[:-1]]).astype(np.int32)
        d2 = np.concatenate([[ninf, ninf], d[:-2]])[:S].astype(dtype)
        s2 = np.concatenate([[-1, -1], st[:-2]])[:S].astype(np.int32)
        m, b = d.copy(), st.copy()
        g = d1 > m
        m[g], b[g] = d1[g], s1[g]
        g = skip & (d2 > m)
        m[g], b[g] = d2[g], s2[g]
        if dtype(0) > m[0]:
            m[0], b[0] = dtype(0), t
        d = (m + r[t]).astype(dtype)
        st = np.where(d == ninf, -1, b).astype(np.int32)
        trace[t], tstart[t] = d[S - 1], st[S - 1]
        if d[S - 1] >= best:
            best, bt, bs = d[S - 1], t, int(st[S - 1])
    if best == ninf:
        return ninf, -1, -1, trace, tstart
    return best, bs, bt + 1, trace, tstart


def spot_batch(logp, tlen, top, keywords, blank=0, V=None, Lmax=None, dtype=np.float32):
    """logp (U, Tm, >= V), tlen (U,), top (U, Tm) or None, keywords a list of K id sequences ->
    score (U, K) dtype, start, end (U, K) int32, trace (U, K, Tm) dtype, tstart (U, K, Tm) int32:
    the outputs of avsr_ctc_kws"""
    logp = np.asarray(logp)
    U, Tm = logp.shape[:2]
    K = len(keywords)
    score = np.empty((U, K), dtype=dtype)
    start = np.empty((U, K), dtype=np.int32)
    end = np.empty((U, K), dtype=np.int32)
    trace = np.empty((U, K, Tm), dtype=dtype)
    tstart = np.empty((U, K, Tm), dtype=np.int32)
    for u in range(U):
        for k, y in enumerate(keywords):
            score[u, k], start[u, k], end[u, k], trace[u, k], tstart[u, k] = spot(
                logp[u], y, int(tlen[u]), None if top is None else np.asarray(top)[u], blank, V, Lmax, Tm, dtype)
    return score, start, end, trace, tstart


def pinned(r, ext, skip):
    """fp64 CTC Viterbi score of the path that is in state 0 at the first row of r (n, S) and in
    state S - 1 at its last; -inf when there is none"""
    n, S = r.shape
    d = np.full(S, -np.inf)
    d[0] = r[0, 0]
    for t in range(1, n):
        c = d.copy()
        c[1:] = np.maximum(c[1:], d[:-1])
        c[2:] = np.maximum(c[2:], np.where(skip[2:], d[:-2], -np.inf))
        d = c + r[t]
    return d[S - 1]


def brute_force(logp, y, n, top=None, blank=0):
    """fp64 maximum over all spans [s, e) of the pinned Viterbi of y over frames s .. e-1"""
    y = [int(t) for t in y]
    S = 2 * len(y) - 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[0::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    lp = np.asarray(logp, dtype=np.float64)[:n]
    f = np.zeros(n) if top is None else lp[np.arange(n), np.asarray(top)[:n]]
    r = lp[:, ext] - f[:, None]
    best = -np.inf
    for s in range(n):
        for e in range(s + 1, n + 1):
            best = max(best, pinned(r[s:e], ext, skip))
    return best

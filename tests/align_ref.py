"""Plain numpy CTC Viterbi with exactly the recursion, roundings and tie order of
avsr_ctc_align (include/avsr_hip.h), vectorised over the states. A helper, not a test: in
float32 it reproduces the kernel bit for bit; `dtype=np.float64` gives the fp64 Viterbi of the
same emissions.

  ext = blank, y1, blank, ..., yL, blank                       S = 2L + 1 states
  e(t, s) = dtype(x[t][ext_s]) - dtype(lse[t])
  d[0][0] = e(0, 0), d[0][1] = e(0, 1), every other state -inf
  d[t][s] = max(c0, c1, c2) + e(t, s)
      c0 = d[t-1][s];  c1 = d[t-1][s-1] (s >= 1, no wrap-around);
      c2 = d[t-1][s-2] (s >= 2, ext_s != blank, ext_s != ext_{s-2})
  back-pointer: the first maximum in the order (s, s-1, s-2)
  final state: the first maximum of (S-2, S-1); state 0 for L = 0
"""
import numpy as np


def viterbi(x, lse, y, T, blank=0, dtype=np.float32):
    """one utterance: x (>= T, >= V) logits (or log-probs with lse = 0), lse (>= T,), y the label
    ids, T its frames -> (ali int32 (T,), score, feasible); infeasible: (all -1, 0, 0)"""
    y = np.asarray(y, dtype=np.int64).reshape(-1)
    S = 2 * len(y) + 1
    if T <= 0:
        return np.full(max(T, 0), -1, np.int32), dtype(0), 0
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = y
    e = np.asarray(x)[:T][:, ext].astype(dtype) - np.asarray(lse)[:T, None].astype(dtype)
    assert e.dtype == dtype
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = dtype(-np.inf)
    d = np.full(S, ninf, dtype=dtype)
    d[:2] = e[0, :2]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        c1 = np.concatenate([[ninf], d[:-1]]).astype(dtype)
        c2 = np.where(skip, np.concatenate([[ninf, ninf], d[:-2]])[:S], ninf).astype(dtype)
        m = d.copy()
        k = np.zeros(S, dtype=np.int8)
        g = c1 > m
        m[g], k[g] = c1[g], 1
        g = c2 > m
        m[g], k[g] = c2[g], 2
        d = m + e[t]
        bp[t] = k
    s = 0 if S == 1 else (S - 1 if d[S - 1] > d[S - 2] else S - 2)
    if not d[s] > ninf:
        return np.full(T, -1, np.int32), dtype(0), 0
    score = d[s]
    ali = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        ali[t] = ext[s]
        if t > 0:
            s -= int(bp[t, s])
    return ali, score, 1


def align_batch(x, lse, labels, in_len, T, blank=0, dtype=np.float32):
    """x (B*T, >= V) rows b*T + t, lse (B*T,), labels a list of B id sequences, in_len (B,) ->
    ali (B, T) int32 (-1 at t >= in_len[b]), score (B,) dtype, feasible (B,) int32: the outputs
    of avsr_ctc_align"""
    B = len(labels)
    ali = np.full((B, T), -1, dtype=np.int32)
    score = np.zeros(B, dtype=dtype)
    feas = np.zeros(B, dtype=np.int32)
    x, lse = np.asarray(x), np.asarray(lse)
    for b in range(B):
        Tb = min(int(in_len[b]), T)
        a, sc, f = viterbi(x[b * T:(b + 1) * T], lse[b * T:(b + 1) * T], labels[b], Tb, blank, dtype)
        if f:
            ali[b, :Tb], score[b], feas[b] = a, sc, 1
    return ali, score, feas

"""Frame-at-a-time float32 CTC Viterbi with gap states: the definition of avsr_ctc_align_gaps in
include/avsr_hip.h, restated on tests/align_long_ref.viterbi. A flagged blank state (position i of
`gap` is state 2 i) emits ef = filler[t] + gap_penalty where ef > eb = x[t][blank] - lse[t]
(strictly), else eb; a frame spent that way is GAP (-2) in ali. Nothing else differs. A helper, not
a test; tests/test_align_gaps_ref.py checks it. Also the planted inputs that the CPU and the GPU
tests share."""
import numpy as np

GAP = -2


def _ef(filler, t, gap_penalty):
    return np.float32(np.float32(filler[t]) + np.float32(gap_penalty))      # ONE fp32 add


def viterbi(x, lse, filler, y, gap, gap_penalty, T, blank=0):
    """one recording: x (>= T, >= V) float32 logits, lse and filler (>= T,) float32, y the label
    ids, gap len(y) + 1 flags, T its frames -> (ali int32 (T,), score float32, feasible);
    infeasible: (all -1, 0, 0)"""
    f32 = np.float32
    x, lse, filler = np.asarray(x), np.asarray(lse), np.asarray(filler)
    assert x.dtype == f32 and lse.dtype == f32 and filler.dtype == f32
    y = np.asarray(y, dtype=np.int64).reshape(-1)
    S = 2 * len(y) + 1
    if T <= 0:
        return np.full(max(T, 0), -1, np.int32), f32(0), 0
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = y
    g = np.zeros(S, dtype=bool)
    g[0::2] = np.asarray(gap)[:len(y) + 1] != 0
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = f32(-np.inf)

    def emissions(t):
        e = x[t, ext] - lse[t]
        ef = _ef(filler, t, gap_penalty)
        e[g & (ef > e)] = ef
        assert e.dtype == f32
        return e

    d = np.full(S, ninf, dtype=f32)
    d[:2] = emissions(0)[:2]
    bp = np.zeros((T, S), dtype=np.uint8)
    for t in range(1, T):
        e = emissions(t)
        m = d.copy()
        k = bp[t]
        c = d[:-1] > m[1:]                        # c1 > c0
        m[1:][c] = d[:-1][c]
        k[1:][c] = 1
        c2 = np.where(skip[2:], d[:-2], ninf)
        c = c2 > m[2:]
        m[2:][c] = c2[c]
        k[2:][c] = 2
        d = m + e
        assert d.dtype == f32
    s = 0 if S == 1 else (S - 1 if d[S - 1] > d[S - 2] else S - 2)
    if not d[s] > ninf:
        return np.full(T, -1, np.int32), f32(0), 0
    score = d[s]
    ali = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        ali[t] = ext[s]
        if g[s] and _ef(filler, t, gap_penalty) > x[t, blank] - lse[t]:
            ali[t] = GAP
        if t > 0:
            s -= int(bp[t, s])
    return ali, score, 1


def align_batch(x, lse, filler, labels, gaps, gap_penalty, in_len, T, blank=0):
    """the outputs of avsr_ctc_align_gaps for x (B*T, >= V) float32 rows b*T + t, lse and filler
    (B*T,): ali (B, T) int32, score (B,) float32, feasible (B,) int32. gaps[b]: len(labels[b]) + 1
    flags"""
    B = len(labels)
    ali = np.full((B, T), -1, dtype=np.int32)
    score = np.zeros(B, dtype=np.float32)
    feas = np.zeros(B, dtype=np.int32)
    for b in range(B):
        Tb = min(int(in_len[b]), T)
        r = slice(b * T, (b + 1) * T)
        a, sc, f = viterbi(x[r], lse[r], filler[r], labels[b], gaps[b], gap_penalty, Tb, blank)
        if f:
            ali[b, :Tb], score[b], feas[b] = a, sc, 1
    return ali, score, feas


def frame_terms(x, lse, filler, gap_penalty, ali):
    """the path's own float32 term per frame: filler[t] + gap_penalty at GAP frames, else
    x[t][ali[t]] - lse[t]"""
    f32 = np.float32
    x, lse, filler = np.asarray(x), np.asarray(lse), np.asarray(filler)
    assert x.dtype == f32 and lse.dtype == f32 and filler.dtype == f32
    ali = np.asarray(ali, dtype=np.int64)
    n = len(ali)
    e = x[np.arange(n), np.where(ali == GAP, 0, ali)] - lse[:n]
    ef = filler[:n] + f32(gap_penalty)
    e[ali == GAP] = ef[ali == GAP]
    assert e.dtype == f32
    return e


def path_sum(x, lse, filler, gap_penalty, ali):
    """the sequential float32 sum of frame_terms: what the score is, bit for bit (one emission is
    added per frame, in frame order)"""
    e = frame_terms(x, lse, filler, gap_penalty, ali)
    acc = e[0]
    for v in e[1:]:
        acc = np.float32(acc + v)
    return acc


def random_flags(L, seed, p=0.3):
    """L + 1 flags, each set with probability p (positions 0 and L included)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.random(L + 1) < p).astype(np.uint8)


def filler_of(x, lse, V):
    """the greedy reading max_v x[t][v] - lse[t] over the V valid columns, float32"""
    return (np.asarray(x)[:, :V].max(1) - np.asarray(lse)).astype(np.float32)


# the two planted cases: (segments, flags set, T); a segment is (first frame, tokens)
Y8 = (5, 17, 30, 42, 40, 9, 11, 3)
FREE_ENDS = dict(segments=[(40, Y8)], T=120, seed=1, y=Y8, flags=(0, 8))
MID_GAP = dict(segments=[(10, Y8[:4]), (70, Y8[4:])], T=120, seed=2, y=Y8, flags=(0, 4, 8))


def planted(segments, T, seed, V=64):
    """float32 logits (T, V), lse, filler (the row maximum - lse) and {token index in the
    concatenated transcript: (first, last + 1) of its three planted frames}. Every frame is
    N(0, 1) noise with one column raised by 8: in a segment (first frame, tokens) each token for 3
    frames, then blank (0) for 2; on every other frame a random non-blank token, "speech" that the
    transcript does not cover."""
    f32 = np.float32
    r = np.random.Generator(np.random.PCG64(seed))
    x = r.normal(size=(T, V)).astype(f32)
    peak = r.integers(1, V, size=T)
    x[np.arange(T), peak] += 8
    truth, n = {}, 0
    for first, toks in segments:
        t = first
        for k in toks:
            truth[n] = (t, t + 3)
            n += 1
            for col in (k, k, k, 0, 0):
                x[t] = r.normal(size=V)
                x[t, col] += 8
                t += 1
        assert t <= T
    lse = np.log(np.exp(x.astype(np.float64)).sum(1)).astype(f32)
    return x, lse, filler_of(x, lse, V), truth


def flags_at(L, positions):
    g = np.zeros(L + 1, dtype=np.uint8)
    g[list(positions)] = 1
    return g


def gap_runs(ali):
    """maximal [start, end) runs of GAP in ali"""
    a = np.concatenate([[0], (np.asarray(ali) == GAP).astype(np.int8), [0]])
    d = np.diff(a)
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))

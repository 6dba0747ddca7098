"""Frame-at-a-time float32 CTC Viterbi for long label sequences: the arithmetic and tie order of
tests/align_ref.viterbi (the definition of avsr_ctc_align and avsr_ctc_align_long in
include/avsr_hip.h), but it gathers ONE frame's emissions at a time, so its memory is T * S bytes
of back-pointers and not T * S * 4 of emissions. A helper, not a test; tests/test_align_long_ref.py
shows that it equals align_ref.viterbi. Also the inputs and the launch cases that the CPU and the
GPU tests of the long kernel share (the four launches of tests/test_gpu_align.py)."""
import numpy as np
import torch

BIG = 1e30          # fills every column >= V and every frame >= in_len[b]: a stray read shows

# (T_b, labels) pairs; ids < 64 so they serve V = 64: launches 1-4 of tests/test_gpu_align.py
Y6, Y4 = (5, 17, 30, 42, 40, 9), (7, 47, 1, 2)
LAUNCH1 = [(25, Y6), (19, Y4), (12, (7, 7, 7, 3, 3)), (7, (9, 9, 9, 9)), (6, (1, 2, 3, 4, 5, 6)), (40, (11,)),
           (1, (4,)), (5, ())]
LAUNCH2 = [(12, (7, 7, 7, 3, 3)), (6, (9, 9, 9, 9)), (25, Y6), (3, (1, 2, 3, 4)), (0, (4,)), (7, (9, 9, 9, 9))]
LAUNCH4 = [(9, (3, 3, 5))]


def launch3():
    """S = 261 and S = 1023, with a few adjacent repeats (one triple)"""
    rng = np.random.Generator(np.random.PCG64(5))
    y130 = rng.integers(1, 64, size=130).tolist()
    for i in (10, 11, 50, 100):
        y130[i + 1] = y130[i]
    y511 = rng.integers(1, 64, size=511).tolist()
    assert 511 + sum(a == b for a, b in zip(y511, y511[1:])) <= 600
    return [(300, tuple(y130)), (600, tuple(y511))]


def launches():
    """[(name, cases, T, kwargs of inputs())]"""
    return [("ragged", LAUNCH1, 40, dict(seed=0)), ("infeasible", LAUNCH2, 25, dict(seed=1)),
            ("states", launch3(), 600, dict(seed=2)), ("ties0", LAUNCH4, 9, dict(const=0.0)),
            ("ties-1.7", LAUNCH4, 9, dict(const=-1.7))]


def random_labels(L, seed, repeats=(), hi=64, distinct=False):
    """L ids in [1, hi); repeats: indices i with y[i + 1] = y[i]; distinct: no two neighbours equal"""
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(1, hi, size=L)
    if distinct:
        for i in range(1, L):
            if y[i] == y[i - 1]:
                y[i] = 1 + (y[i] % (hi - 1))            # another id in [1, hi)
        assert not (y[1:] == y[:-1]).any()
    for i in repeats:
        y[i + 1] = y[i]
    return tuple(int(v) for v in y)


def n_repeats(y):
    return sum(a == b for a, b in zip(y, y[1:]))


def inputs(cases, T, V, ldx, dtype, seed=0, const=None, quant=None):
    """logits (B*T, ldx) of `dtype` (random, all `const`, or random multiples of `quant`) with BIG
    outside the valid region, and the fp32 row log-sum-exp of the upcast values"""
    B = len(cases)
    if const is None:
        x = torch.randn(B * T, ldx, generator=torch.Generator().manual_seed(seed)) * 3
        if quant:
            x = torch.round(x / quant) * quant
    else:
        x = torch.full((B * T, ldx), float(const))
    x[:, V:] = BIG
    for b, (Tb, _) in enumerate(cases):
        x[b * T + max(Tb, 0):(b + 1) * T] = BIG
    x = x.to(dtype)
    lse = torch.logsumexp(x.float()[:, :V], -1)
    return x, lse


def viterbi(x, lse, y, T, blank=0):
    """one recording: x (>= T, >= V) float32 logits, lse (>= T,), y the label ids, T its frames
    -> (ali int32 (T,), score float32, feasible); infeasible: (all -1, 0, 0)"""
    f32 = np.float32
    x, lse = np.asarray(x), np.asarray(lse)
    assert x.dtype == f32 and lse.dtype == f32
    y = np.asarray(y, dtype=np.int64).reshape(-1)
    S = 2 * len(y) + 1
    if T <= 0:
        return np.full(max(T, 0), -1, np.int32), f32(0), 0
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = f32(-np.inf)
    d = np.full(S, ninf, dtype=f32)
    d[:2] = x[0, ext[:2]] - lse[0]
    bp = np.zeros((T, S), dtype=np.uint8)
    for t in range(1, T):
        e = x[t, ext] - lse[t]
        m = d.copy()
        k = bp[t]
        g = d[:-1] > m[1:]                        # c1 > c0
        m[1:][g] = d[:-1][g]
        k[1:][g] = 1
        c2 = np.where(skip[2:], d[:-2], ninf)
        g = c2 > m[2:]
        m[2:][g] = c2[g]
        k[2:][g] = 2
        d = m + e
        assert d.dtype == f32
    s = 0 if S == 1 else (S - 1 if d[S - 1] > d[S - 2] else S - 2)
    if not d[s] > ninf:
        return np.full(T, -1, np.int32), f32(0), 0
    score = d[s]
    ali = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        ali[t] = ext[s]
        if t > 0:
            s -= int(bp[t, s])
    return ali, score, 1


def align_batch(x, lse, labels, in_len, T, blank=0):
    """the outputs of avsr_ctc_align_long for x (B*T, >= V) float32 rows b*T + t: ali (B, T) int32,
    score (B,) float32, feasible (B,) int32"""
    B = len(labels)
    ali = np.full((B, T), -1, dtype=np.int32)
    score = np.zeros(B, dtype=np.float32)
    feas = np.zeros(B, dtype=np.int32)
    for b in range(B):
        Tb = min(int(in_len[b]), T)
        a, sc, f = viterbi(x[b * T:(b + 1) * T], lse[b * T:(b + 1) * T], labels[b], Tb, blank)
        if f:
            ali[b, :Tb], score[b], feas[b] = a, sc, 1
    return ali, score, feas


def path_sum(x, lse, ali):
    """the sequential float32 sum over t of x[t][ali[t]] - lse[t]: what a Viterbi score is, bit for
    bit, because d[t] = max(...) + e(t, s) adds one emission per frame in frame order"""
    f32 = np.float32
    x, lse = np.asarray(x), np.asarray(lse)
    assert x.dtype == f32 and lse.dtype == f32
    e = x[np.arange(len(ali)), np.asarray(ali, dtype=np.int64)] - lse[:len(ali)]
    acc = e[0]
    for v in e[1:]:
        acc = f32(acc + v)
    return acc

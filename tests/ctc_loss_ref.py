"""Plain CTC forward-backward on the CPU, written from the statement of avsr_ctc_fwd / avsr_ctc_bwd
in include/avsr_hip.h and the textbook recursion (Graves et al. 2006), plus the case tables that
tests/test_ctc_loss_ref.py (CPU) and tests/test_gpu_loss_edges.py (GPU) share. A helper, not a test.

  ext = blank, y1, blank, y2, ..., yL, blank                      S = 2L + 1 states, blank = 0
  lp(t, s) = log softmax(logits[t])[ext_s]
  alpha_0(s) = lp(0, s) for s < 2, else -inf
  alpha_t(s) = lp(t, s) + log(e^alpha_{t-1}(s) + e^alpha_{t-1}(s-1) + [skip(s)] e^alpha_{t-1}(s-2))
  skip(s): ext_s is a label and differs from ext_{s-2}
  log P = log(e^alpha_{Tb-1}(S-1) + e^alpha_{Tb-1}(S-2)),  nll = -log P,  Tb = min(in_len, T)
  beta is the mirror image (its own emission included), so
  gamma_t(s) = exp(alpha_t(s) + beta_t(s) - lp(t, s) - log P) = P(path in state s at t | x)
  grad[t][k] = softmax_t(k) - sum_{s: ext_s = k} gamma_t(s)      (d nll / d logits, t < Tb)
No path, or in_len <= 0: every output is 0 (zero_infinity).
"""
import functools

import torch
import torch.nn.functional as F


def _lse3(a, b, c):
    return torch.logsumexp(torch.stack([a, b, c]), dim=0)      # all -inf -> -inf, no NaN


def ctc_ref(logits, labels, in_len, dtype=torch.float64):
    """logits (T, V) -> nll (0-dim), alpha (Tb, S), gamma (T, S), grad (T, V), all in `dtype`:
    float64 is the reference, float32 the same recursion in fp32 (its own rounding error)."""
    T, V = logits.shape
    labels = [int(k) for k in labels]
    L, S = len(labels), 2 * len(labels) + 1
    Tb = max(0, min(int(in_len), T))

    def nothing():
        return (torch.zeros((), dtype=dtype), torch.zeros(Tb, S, dtype=dtype), torch.zeros(T, S, dtype=dtype),
                torch.zeros(T, V, dtype=dtype))

    if Tb == 0:
        return nothing()
    ext = torch.zeros(S, dtype=torch.long)
    ext[1::2] = torch.tensor(labels, dtype=torch.long)
    skip = torch.zeros(S, dtype=torch.bool)
    skip[2:] = (torch.arange(S)[2:] & 1).bool() & (ext[2:] != ext[:-2])
    logsm = torch.log_softmax(logits[:Tb].to(dtype), dim=1)
    lp = logsm[:, ext]                                          # (Tb, S)
    ninf = torch.full((S + 2,), float("-inf"), dtype=dtype)

    def down(v, k):        # v[s - k], -inf below state 0
        return torch.cat([ninf[:k], v])[:S]

    def up(v, k):          # v[s + k], -inf past state S - 1
        return torch.cat([v, ninf[:k]])[k:]

    alpha = torch.full((Tb, S), float("-inf"), dtype=dtype)
    alpha[0, :2] = lp[0, :2]
    for t in range(1, Tb):
        a = alpha[t - 1]
        alpha[t] = _lse3(a, down(a, 1), torch.where(skip, down(a, 2), ninf[:S])) + lp[t]
    logp = torch.logsumexp(alpha[Tb - 1, max(S - 2, 0):], dim=0)
    if logp == float("-inf"):
        return nothing()
    skip_up = torch.cat([skip, torch.zeros(2, dtype=torch.bool)])[2:]        # skip(s + 2)
    beta = torch.full((Tb, S), float("-inf"), dtype=dtype)
    beta[Tb - 1, max(S - 2, 0):] = lp[Tb - 1, max(S - 2, 0):]
    for t in range(Tb - 2, -1, -1):
        b = beta[t + 1]
        beta[t] = _lse3(b, up(b, 1), torch.where(skip_up, up(b, 2), ninf[:S])) + lp[t]
    gamma = torch.zeros(T, S, dtype=dtype)
    gamma[:Tb] = torch.exp(alpha + beta - lp - logp)
    grad = torch.zeros(T, V, dtype=dtype)
    grad[:Tb] = torch.exp(logsm) - torch.zeros(Tb, V, dtype=dtype).index_add_(1, ext, gamma[:Tb])
    return -logp, alpha, gamma, grad


def torch_ctc(logits, labels, in_len, dtype):
    """torch.nn.functional.ctc_loss (blank 0, zero_infinity) of one utterance in `dtype` on the CPU:
    logits (T, V) -> nll (0-dim), d nll / d logits (T, V). Needs 1 <= in_len; in_len is cut to T."""
    T = logits.shape[0]
    x = logits.to(dtype).unsqueeze(1).clone().requires_grad_()
    nll = F.ctc_loss(x.log_softmax(-1), torch.tensor([labels], dtype=torch.long).view(1, -1),
                     torch.tensor([min(int(in_len), T)]), torch.tensor([len(labels)]), blank=0,
                     reduction="none", zero_infinity=True)
    nll.sum().backward()
    return nll.detach()[0], x.grad[:, 0]


def feasible(labels, in_len, T):
    n = min(int(in_len), T)
    return n >= 1 and n >= len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))


# ------------------------------------------------------------------------------ case tables
def _cycle(n, hi):
    return [1 + i % hi for i in range(n)]


# name -> T, V, ldx (logits row stride), lddx (gradient row stride), utterances (labels, in_len).
# avsr_ctc_fwd gathers CH = max(1, min(64, 6144 / S)) frames of emissions at a time, S = 2L + 1.
CTC_CASES = {
    # no recursion step; the final lse2 over the last two states; [5, 6] has no path in one frame
    "one-frame": dict(T=1, V=9, ldx=16, lddx=16, utts=[([], 1), ([5], 1), ([5, 6], 1)]),
    # L = 0; a single path ([2,2,2]@5, [1..8]@8) and one frame short of it; empty input;
    # in_len > T; a second chunk of 6 frames (T = 70, CH = 64)
    "short": dict(T=70, V=9, ldx=16, lddx=24,
                  utts=[([], 70), ([1], 1), ([2, 2, 2], 5), (_cycle(8, 8), 8), ([2, 2, 2], 4), (_cycle(8, 8), 7),
                        ([1, 2], 0), ([1, 2], 75)]),
    # S = 95 (CH = 64) and S = 97 (CH = 63): both sides of min(64, 6144 / S); input of one chunk,
    # one frame more, 2 CH + 1
    "chunk-edges": dict(T=129, V=50, ldx=56, lddx=64,
                        utts=[(_cycle(47, 49), 64), (_cycle(47, 49), 65), (_cycle(47, 49), 129),
                              (_cycle(48, 49), 63), (_cycle(48, 49), 64), (_cycle(48, 49), 127)]),
    # S = 1023 (CH = 6, 4 states per thread); S = 257; S = 511 without any skip transition, tight
    # (509 frames) and one frame short; ctc_bwd's label loop with L > 256; ldx == V
    "wide": dict(T=520, V=40, ldx=40, lddx=48,
                 utts=[(_cycle(511, 39), 520), (_cycle(128, 39), 300), ([3] * 255, 509), ([3] * 255, 508)]),
    # V = 2: one label, V below one vector
    "two-symbols": dict(T=65, V=2, ldx=8, lddx=8, utts=[([1] * 30, 65), ([1], 64)]),
    # production V
    "vocab": dict(T=8, V=5049, ldx=5056, lddx=5064, utts=[([5, 5, 17, 5047], 8), ([1], 3)]),
}
CONFIDENT_CASES = ("chunk-edges", "wide")
REGIMES = ("random", "match", "mismatch")
JUNK = 60.0           # rows t >= in_len: +-60 alternating (exact in bf16)


def planted_alignment(labels, n):
    """a valid CTC path of `labels` cut / padded to n frames: one frame per label, a blank
    between adjacent equal labels, blanks to the end"""
    seq, prev = [], None
    for k in labels:
        if k == prev:
            seq.append(0)
        seq.append(k)
        prev = k
    return (seq + [0] * n)[:n]


@functools.lru_cache(maxsize=None)
def case_logits(name, regime, dtype=torch.float32):
    """the logits of a case as stored on the device: (B, T, ldx) in `dtype` (rounded once, here).
    Columns V.. hold NaN, rows t >= in_len hold +-60. regime: "random" = randn * 2; "match" /
    "mismatch" = randn + 12 * onehot(planted symbol of frame t), planted from the labels / from
    the labels shifted by one symbol (1 + k % (V - 1)). Shared: do not write to the result."""
    c = CTC_CASES[name]
    T, V, ldx, utts = c["T"], c["V"], c["ldx"], c["utts"]
    g = torch.Generator().manual_seed(1000 + sorted(CTC_CASES).index(name) * 10 + REGIMES.index(regime))
    x = torch.full((len(utts), T, ldx), float("nan"))
    x[:, :, :V] = torch.randn(len(utts), T, V, generator=g) * (2 if regime == "random" else 1)
    col = torch.arange(V)
    for b, (labels, in_len) in enumerate(utts):
        n = max(0, min(in_len, T))
        if regime != "random":
            plant = labels if regime == "match" else [1 + k % (V - 1) for k in labels]
            ali = torch.tensor(planted_alignment(plant, n), dtype=torch.long)
            x[b, torch.arange(n), ali] += 12.0
        for t in range(n, T):
            x[b, t, :V] = JUNK * (1 - 2 * ((col + t) & 1)).float()
    return x.to(dtype)


def all_ctc_cases():
    """(name, regime) of every CTC case: each shape case with random logits, the confident ones twice more"""
    return [(n, "random") for n in CTC_CASES] + [(n, r) for n in CONFIDENT_CASES for r in ("match", "mismatch")]

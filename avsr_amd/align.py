"""When each token / word was said: CTC forced alignment of hypotheses on the HIP engine.

The frame alignment is the Viterbi path of the reference's CTC.forced_align_batch
(src/nets/backend/ctc.py:246-328), computed on the device by avsr_ctc_align (one launch for a
batch of utterances, logits never leave the device); this module turns it into what callers
use: token spans and word times.

    spans = align_batch(model.avsr, [enc_u for ...], [hyp.yseq for ...])
    words = word_times(spans[0].spans, token_list, frame_rate=cfg.label_rate)
"""
from collections import namedtuple

import torch

from . import ops

TokenSpan = namedtuple("TokenSpan", ["token", "start", "end"])        # frames [start, end)
Alignment = namedtuple("Alignment", ["spans", "score"])               # score: log-probability of the path


def token_spans(ali, blank=0):
    """collapse a frame alignment (token id per frame) into TokenSpans: a maximal run of one
    non-blank id is one token (CTC separates adjacent equal labels by a blank, so a run never
    holds two tokens); blank frames belong to no span"""
    spans = []
    prev, start = blank, 0
    ali = [int(a) for a in ali]
    for t, a in enumerate(ali):
        if a != prev:
            if prev != blank:
                spans.append(TokenSpan(prev, start, t))
            prev, start = a, t
    if prev != blank:
        spans.append(TokenSpan(prev, start, len(ali)))
    return spans


def strip_sos_eos(yseq, sos, eos):
    """token ids of a Hypothesis.yseq without its leading sos and trailing eos"""
    y = [int(t) for t in yseq]
    if y and y[0] == sos:
        y = y[1:]
    if y and y[-1] == eos:
        y = y[:-1]
    return y


@torch.no_grad()
def align_batch(e2e, xs, yseqs):
    """Forced alignment of U utterances: xs = list of encoded utterances (T_u, D), yseqs = list
    of token-id sequences (a leading sos / trailing eos, as in Hypothesis.yseq, is stripped).
    Returns per utterance Alignment(spans, score), or None where no alignment exists (fewer
    frames than labels + adjacent repeats: a beam hypothesis can be infeasible).

    The CTC logits are computed per utterance (M = T_u rows per GEMM launch, as
    BatchBeamSearch.decode_batch does for the same reason: the few-row and tiled GEMM cores
    round differently, so one launch over the padded batch would make an utterance's result
    depend on the batch); then ONE avsr_ctc_align launch aligns the padded batch."""
    if len(xs) != len(yseqs):
        raise ValueError(f"{len(xs)} utterances but {len(yseqs)} token sequences")
    U = len(xs)
    if U == 0:
        return []
    eng = e2e.engine()
    dev = eng.device
    ys = [strip_sos_eos(y, e2e.sos, e2e.eos) for y in yseqs]
    Ts = [int(x.shape[0]) for x in xs]
    Tm, D = max(Ts), eng.D
    xp = torch.zeros(U, Tm, D, device=dev, dtype=eng.dtype)
    cl = torch.zeros(U * Tm, eng.Vp, device=dev, dtype=eng.dtype)
    for u, x in enumerate(xs):
        if Ts[u] == 0:
            continue
        ops.cast(x.to(dev).reshape(Ts[u], D).contiguous(), xp[u, :Ts[u]])
        ops.linear_fwd(xp[u, :Ts[u]], eng.w("ctc.ctc_lo.weight"), eng.arena.master("ctc.ctc_lo.bias"),
                       out=cl[u * Tm:u * Tm + Ts[u], :eng.V])
    ali, score, feas = _align_logits(eng, cl, U, Tm, ys, Ts, e2e.blank)
    out = []
    for u in range(U):
        out.append(Alignment(token_spans(ali[u, :Ts[u]], e2e.blank), float(score[u])) if feas[u] else None)
    return out


def _align_logits(eng, logits, B, T, ys, ilens, blank):
    """avsr_ctc_align over logits (B*T, >= V) on the device -> host (ali (B, T) int32,
    score (B,) fp32, feasible (B,) int32)"""
    dev = logits.device
    for b, y in enumerate(ys):
        if any(t < 0 or t >= eng.V for t in y):
            raise ValueError(f"utterance {b}: token id outside [0, {eng.V})")
    Lmax = max(1, max(len(y) for y in ys))
    lab = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, y in enumerate(ys):
        lab[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
    lse = torch.empty(B * T, device=dev, dtype=torch.float32)
    ops.row_lse(logits, eng.V, lse)
    ali, score, feas = ops.ctc_align(logits, B, T, eng.V, lab.to(dev),
                                     torch.tensor([len(y) for y in ys], dtype=torch.int32).to(dev),
                                     torch.tensor([int(t) for t in ilens], dtype=torch.int32).to(dev), lse, blank=blank)
    return ali.cpu().numpy(), score.cpu().numpy(), feas.cpu().numpy()


def word_groups(tokens, token_list, space="▁"):
    """[(word, [indices into tokens])] of sentence-piece ids: a word starts at a piece that begins
    with `space` (and at the first piece) and runs to its last piece. The one word segmentation of
    word_times and avsr_amd.confidence.word_confidences, so that their lists zip."""
    words = []
    for i, tok in enumerate(tokens):
        piece = token_list[int(tok)]
        if piece.startswith(space) or not words:
            words.append([piece[len(space):] if piece.startswith(space) else piece, [i]])
        else:
            words[-1][0] += piece
            words[-1][1].append(i)
    return [(w, idx) for w, idx in words]


def word_times(spans, token_list, frame_rate=25.0, space="▁"):
    """(word, start_s, end_s) from TokenSpans of sentence pieces: a word starts at a piece that
    begins with `space` (and at the first piece), runs to the end of its last piece; times are
    frames / frame_rate (the config's label_rate)."""
    return [(w, spans[idx[0]].start / frame_rate, spans[idx[-1]].end / frame_rate)
            for w, idx in word_groups([sp.token for sp in spans], token_list, space)]

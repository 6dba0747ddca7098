"""Whole transcripts against whole recordings: long-form CTC alignment on the HIP engine.

Every other entry point here works on one clip of at most 15 s (375 frames, the training maximum).
This module aligns the untimed transcript of a recording of many minutes to the whole recording,
and cuts the recording into clips of at most 15 s at its pauses, each with its text: training
clips, or the word times of a caption file.

    videos, audios = ...                       # (1, 1, T, 88, 88), (1, 104, T): frontend.collate
    logits, lse = ctc_logits_long(model.avsr, videos, audios)
    a = align_long(model.avsr, logits, lse, y)                 # y: the transcript's token ids
    words = align.word_times(a.spans, token_list, frame_rate=cfg.label_rate)
    clips = segments(a, token_list, max_frames=375)
    good = [s for s in clips if s.end - s.start <= 375 and s.worst > threshold]

* The encoder was trained on clips of at most 375 frames and its attention is quadratic in T, so
  the recording is encoded in overlapping windows of `window` frames (window_plan); of each window
  only the middle is kept, so that every kept frame has context on both sides. `overlap` = 125
  frames (5 s, at least 2.5 s of context on either side) is a knob: ITS EFFECT ON ACCURACY IS
  UNMEASURED (no checkpoint or data here).
* The alignment is avsr_ctc_align_long (include/avsr_hip.h): the Viterbi of avsr_ctc_align, for up
  to 16383 tokens and any number of frames.
* Segment.score and Segment.worst are mean frame log-probabilities along the alignment. `worst`
  is the figure to threshold where a stretch of the transcript does not match what was said.
  THEIR CALIBRATION IS UNMEASURED, as for avsr_amd.confidence and avsr_amd.kws: tune the threshold
  on held-out data.
* Memory: the stitched logits are T * Vp elements of the engine dtype on the device: for a bf16
  engine T * 5056 * 2 B, 300 MB for 20 minutes (T = 30000). The video tensor itself is larger
  (T * 88 * 88 * 4 B = 930 MB as fp32) and may stay on the host: windows are moved group by group.
  The alignment's back-pointers take T * (2 L + 1) / 4 bytes: 90 MB at T = 30000, L = 6000.
* Out of scope: material at the start or the end of the recording that the transcript does not
  cover (the Viterbi has fixed ends; a free-start variant is a later change); media decoding and
  caption-file writing; transcribing the resulting clips (decode_batch / decode_stream on encoder
  output, as before).
"""
from collections import namedtuple

import numpy as np
import torch

from . import align, ops

MAX_TOKENS = ops.CTC_ALIGN_LONG_LMAX

# spans: align.TokenSpans, one per token of y; score: log-probability of the path; frame_logp:
# (T,) float32 numpy, the path's own log p(ali[t] | x) per frame (it sums to score)
LongAlignment = namedtuple("LongAlignment", ["spans", "score", "frame_logp"])
# frames [start, end) of the recording; first / last: indices into y (inclusive); tokens: their ids;
# text: the words joined by spaces; score / worst: mean frame_logp over the run / of its worst word
Segment = namedtuple("Segment", ["start", "end", "first", "last", "tokens", "text", "score", "worst"])


def window_plan(T, window=375, overlap=125):
    """How a recording of T frames is cut into encoder windows: a list of (start, end, keep_lo,
    keep_hi), frames [start, end) being encoded and [keep_lo, keep_hi) of them kept.

    T <= window: the one window (0, T, 0, T). Otherwise windows start at 0, hop, 2 hop, ... (hop =
    window - overlap) while start + window < T, and one last window (T - window, T) ends the plan,
    so every window is full length. Consecutive windows a, b are cut at c = (b.start + a.end) // 2,
    the middle of their overlap; window i keeps [c_{i-1}, c_i), with 0 and T at the ends. The keeps
    partition [0, T), and a kept frame is at least overlap // 2 frames from any window edge that is
    not an edge of the recording. window = 375 is the training maximum; overlap = 125 (5 s) is
    unmeasured (module docstring)."""
    T, window, overlap = int(T), int(window), int(overlap)
    if T < 1:
        raise ValueError(f"T = {T}: a recording has at least one frame")
    if window < 2:
        raise ValueError(f"window = {window} < 2")
    if overlap < 0 or overlap >= window:
        raise ValueError(f"overlap = {overlap} outside [0, window = {window})")
    if T <= window:
        return [(0, T, 0, T)]
    hop = window - overlap
    starts = list(range(0, T - window, hop)) + [T - window]
    cuts = [0] + [(b + a + window) // 2 for a, b in zip(starts, starts[1:])] + [T]
    return [(s, s + window, cuts[i], cuts[i + 1]) for i, s in enumerate(starts)]


@torch.no_grad()
def ctc_logits_long(e2e, videos, audios, window=375, overlap=125, batch=8):
    """CTC logits of a whole recording: videos (1, 1, T, 88, 88) and audios (1, 104, T) as
    frontend.collate makes them, on the host or the device -> (logits (T, Vp) in the engine dtype,
    lse (T,) fp32, the row log-sum-exp over the V valid columns), both on the device.

    The grouping is the contract (results are bit-equal to doing exactly this by hand): the windows
    of window_plan(T, window, overlap) are encoded `batch` at a time IN PLAN ORDER by ONE
    engine.encode call per group, each with its full length (the last group may be smaller); the
    CTC head then runs ONE WINDOW PER GEMM LAUNCH over the window's rows (as align.align_batch does
    per utterance: the few-row and tiled GEMM cores round differently); rows [keep_lo, keep_hi) of
    each window are copied to the result; ops.row_lse runs once over the stitched rows. With
    T <= window that is engine.encode on the whole recording followed by the head."""
    eng = e2e.engine()
    dev = eng.device
    if videos.dim() != 5 or audios.dim() != 3 or videos.shape[0] != 1 or audios.shape[0] != 1 \
            or videos.shape[2] != audios.shape[2]:
        raise ValueError(f"one recording: videos (1, 1, T, 88, 88) and audios (1, 104, T), got "
                         f"{tuple(videos.shape)} and {tuple(audios.shape)}")
    if int(batch) < 1:
        raise ValueError(f"batch = {batch} < 1")
    T = int(videos.shape[2])
    plan = window_plan(T, window, overlap)
    W = plan[0][1] - plan[0][0]
    logits = torch.zeros(T, eng.Vp, device=dev, dtype=eng.dtype)
    cl = torch.zeros(W, eng.Vp, device=dev, dtype=eng.dtype)
    xw = torch.empty(W, eng.D, device=dev, dtype=eng.dtype)
    for g in range(0, len(plan), int(batch)):
        grp = plan[g:g + int(batch)]
        vid = torch.cat([videos[:, :, s:e] for s, e, _, _ in grp], 0)
        aud = torch.cat([audios[:, :, s:e] for s, e, _, _ in grp], 0)
        enc = eng.encode(aud, vid, torch.full((len(grp),), W, dtype=torch.int64))
        for i, (s, e, lo, hi) in enumerate(grp):
            ops.cast(enc[i].reshape(W, eng.D).contiguous(), xw)
            ops.linear_fwd(xw, eng.w("ctc.ctc_lo.weight"), eng.arena.master("ctc.ctc_lo.bias"), out=cl[:, :eng.V])
            logits[lo:hi] = cl[lo - s:hi - s]
    lse = torch.empty(T, device=dev, dtype=torch.float32)
    ops.row_lse(logits, eng.V, lse)
    return logits, lse


@torch.no_grad()
def align_long(e2e, logits, lse, y):
    """Forced alignment of ONE recording: logits (T, >= V) and lse (T,) from ctc_logits_long, y the
    transcript's token ids (a leading sos / trailing eos is stripped, as in align.align_batch).
    Returns LongAlignment(spans, score, frame_logp), or None where no alignment exists (fewer
    frames than tokens + adjacent repeats). ValueError: ids outside [0, V), blank or eos inside y,
    more than MAX_TOKENS = 16383 tokens. One avsr_ctc_align_long launch; frame_logp[t] =
    float(logits[t][ali[t]]) - lse[t] is gathered on the device."""
    eng = e2e.engine()
    dev = eng.device
    y = align.strip_sos_eos(y, e2e.sos, e2e.eos)
    if any(t < 0 or t >= eng.V for t in y):
        raise ValueError(f"token id outside [0, {eng.V})")
    if any(t == e2e.blank or t == e2e.eos for t in y):
        raise ValueError("blank / eos inside the transcript")
    if len(y) > MAX_TOKENS:
        raise ValueError(f"{len(y)} tokens, avsr_ctc_align_long takes at most {MAX_TOKENS}")
    T = int(logits.shape[0])
    if T < 1 or logits.dim() != 2 or tuple(lse.shape) != (T,):
        raise ValueError(f"logits (T, >= V) and lse (T,), got {tuple(logits.shape)} and {tuple(lse.shape)}")
    lab = torch.full((1, max(1, len(y))), -1, dtype=torch.int32)
    lab[0, :len(y)] = torch.tensor(y, dtype=torch.int32)
    ali, score, feas = ops.ctc_align_long(logits, 1, T, eng.V, lab.to(dev),
                                          torch.tensor([len(y)], dtype=torch.int32).to(dev),
                                          torch.tensor([T], dtype=torch.int32).to(dev), lse, blank=e2e.blank)
    if not int(feas.item()):
        return None
    flp = logits.gather(1, ali.view(T, 1).long()).view(T).float() - lse
    return LongAlignment(align.token_spans(ali[0].cpu().numpy(), e2e.blank), float(score.item()), flp.cpu().numpy())


def segments(alignment, token_list, max_frames=375, margin=5, space="▁"):
    """Cut an aligned recording into clips of at most max_frames frames at its pauses: a list of
    Segments in order, which together hold every token exactly once. Pure host code.

    Words are those of align.word_groups; word i spans [start_i, end_i). The gap after word i is
    g_i = start_{i+1} - end_i and the cut inside it is end_i + g_i // 2. A run of words a..b
    occupies [max(cut_{a-1}, start_a - margin), min(cut_b, end_b + margin)), with 0 and T outside
    the first and the last word: `margin` frames of room around the words, never past the middle of
    a pause. One run holds all words to begin with; a run longer than max_frames with more than one
    word is split at its widest gap (ties: the earliest), until every run fits or is a single word.
    A SINGLE WORD LONGER THAN max_frames IS RETURNED AS IT IS: filter on end - start.
    score = mean of frame_logp over [start_a, end_b); worst = the minimum over the run's words of
    the word's mean frame_logp (calibration unmeasured: module docstring). No tokens: []."""
    spans, flp = alignment.spans, np.asarray(alignment.frame_logp)
    T = len(flp)
    words = align.word_groups([sp.token for sp in spans], token_list, space)
    if not words:
        return []
    start = [spans[idx[0]].start for _, idx in words]
    end = [spans[idx[-1]].end for _, idx in words]
    n = len(words)
    gap = [start[i + 1] - end[i] for i in range(n - 1)]
    cut = [end[i] + gap[i] // 2 for i in range(n - 1)]

    def extent(a, b):
        lo = max(cut[a - 1] if a > 0 else 0, start[a] - margin)
        hi = min(cut[b] if b < n - 1 else T, end[b] + margin)
        return lo, hi

    runs, todo = [], [(0, n - 1)]
    while todo:
        a, b = todo.pop()
        lo, hi = extent(a, b)
        if hi - lo > max_frames and b > a:
            i = max(range(a, b), key=lambda j: (gap[j], -j))
            todo += [(i + 1, b), (a, i)]                # the earlier run is handled first
        else:
            runs.append((a, b, lo, hi))

    def mean(lo, hi):
        return float(np.mean(flp[lo:hi], dtype=np.float64))

    out = []
    for a, b, lo, hi in runs:
        first, last = words[a][1][0], words[b][1][-1]
        out.append(Segment(lo, hi, first, last, [spans[i].token for i in range(first, last + 1)],
                           " ".join(w for w, _ in words[a:b + 1]), mean(start[a], end[b]),
                           min(mean(start[i], end[i]) for i in range(a, b + 1))))
    return out

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
* A transcript that covers only PART of the recording (an intro before the first transcribed
  word, applause after the last, passages the transcriber skipped) goes through align_partial
  (avsr_ctc_align_gaps): the blank before the first token, after the last one and at every listed
  position between two tokens becomes a gap state, which may read a frame as its best token
  (max_v logits[t][v] - lse[t]) plus `gap_penalty` where that beats the blank. Such frames are -2
  in PartialAlignment.ali, their runs are PartialAlignment.gaps, and segments() cuts there and
  keeps clips out of them. `gap_penalty` is a per-frame log-probability and HAS NO DEFAULT: A USEFUL
  VALUE, AND THE ACCURACY OF THE RECOVERED BOUNDARIES ON REAL SPEECH, ARE UNMEASURED (no checkpoint
  or data here).
* Out of scope: transcript words that were NOT SAID (no state is skippable beyond CTC's own rule,
  so these still show as low `worst`); media decoding and caption-file writing; transcribing the
  resulting clips or the uncovered stretches (decode_batch / decode_stream on encoder output, as
  before).
"""
from collections import namedtuple

import numpy as np
import torch

from . import align, ops

MAX_TOKENS = ops.CTC_ALIGN_LONG_LMAX

# spans: align.TokenSpans, one per token of y; score: log-probability of the path; frame_logp:
# (T,) float32 numpy, the path's own log p(ali[t] | x) per frame (it sums to score)
LongAlignment = namedtuple("LongAlignment", ["spans", "score", "frame_logp"])
# align_partial's result. spans, score, frame_logp as above (frame_logp[t] = filler[t] + gap_penalty at a
# gap frame, so it still sums to score); gaps: the maximal runs [start, end) of gap frames, in order; ali:
# (T,) int32 numpy, the token per frame with ops.CTC_ALIGN_GAP = -2 at gap frames
PartialAlignment = namedtuple("PartialAlignment", ["spans", "score", "frame_logp", "gaps", "ali"])
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


def _transcript(e2e, y):
    """y without sos / eos, with align_long's checks but against e2e.odim (the engine's V): no
    device is needed"""
    V = e2e.odim
    y = align.strip_sos_eos(y, e2e.sos, e2e.eos)
    if any(t < 0 or t >= V for t in y):
        raise ValueError(f"token id outside [0, {V})")
    if any(t == e2e.blank or t == e2e.eos for t in y):
        raise ValueError("blank / eos inside the transcript")
    if len(y) > MAX_TOKENS:
        raise ValueError(f"{len(y)} tokens, avsr_ctc_align_long takes at most {MAX_TOKENS}")
    return y


def _frames(logits, lse):
    T = int(logits.shape[0])
    if T < 1 or logits.dim() != 2 or tuple(lse.shape) != (T,):
        raise ValueError(f"logits (T, >= V) and lse (T,), got {tuple(logits.shape)} and {tuple(lse.shape)}")
    return T


def _labels(y, dev):
    lab = torch.full((1, max(1, len(y))), -1, dtype=torch.int32)
    lab[0, :len(y)] = torch.tensor(y, dtype=torch.int32)
    return lab.to(dev), torch.tensor([len(y)], dtype=torch.int32).to(dev)


def gap_flags(n_tokens, free_start=True, free_end=True, gaps=()):
    """the n_tokens + 1 flags of avsr_ctc_align_gaps as a list of 0 / 1: position 0 (free_start),
    position n_tokens (free_end) and the positions `gaps`, i in 1 .. n_tokens - 1 meaning "between
    token i - 1 and token i" (0-based tokens), or "all" for every one of them. ValueError: a
    position outside [1, n_tokens - 1]."""
    L = int(n_tokens)
    flags = [0] * (L + 1)
    if isinstance(gaps, str):
        if gaps != "all":
            raise ValueError(f"gaps = {gaps!r}: positions or 'all'")
        gaps = range(1, L)
    for i in gaps:
        if int(i) != i or i < 1 or i > L - 1:
            raise ValueError(f"gap position {i} outside [1, {L - 1}]")
        flags[int(i)] = 1
    if free_start:
        flags[0] = 1
    if free_end:
        flags[L] = 1
    return flags


def _gap_penalty(gap_penalty):
    g = float(gap_penalty)
    if not g <= 0.0:
        raise ValueError(f"gap_penalty = {gap_penalty}: a log-probability per frame, <= 0 (-inf: no gaps)")
    return g


def gap_runs(ali):
    """maximal [start, end) runs of ops.CTC_ALIGN_GAP in a frame alignment, in order"""
    edge = np.diff(np.concatenate([[0], (np.asarray(ali) == ops.CTC_ALIGN_GAP).astype(np.int8), [0]]))
    return [[int(a), int(b)] for a, b in zip(np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0])]


@torch.no_grad()
def align_partial(e2e, logits, lse, y, *, gap_penalty, free_start=True, free_end=True, gaps=()):
    """align_long for a transcript that covers only part of the recording: the blank before the
    first token (free_start), after the last one (free_end) and at the positions `gaps` (gap_flags:
    i in 1 .. len(y) - 1, "between token i - 1 and token i" of y after sos / eos stripping, or
    "all") is a gap state, which reads frame t as filler[t] + gap_penalty where that is above the
    blank's log-probability; filler[t] = max_v float(logits[t][v]) - lse[t] is computed on the
    device from the engine-dtype logits (exact: the maximum of upcast values is the upcast of their
    maximum; no (T, V) fp32 copy is made). A flagged gap that holds nothing costs nothing.
    gap_penalty <= 0 (-inf: align_long's result) HAS NO DEFAULT: A USEFUL VALUE IS UNMEASURED, as
    is the accuracy of the recovered boundaries on real speech (module docstring).
    Returns PartialAlignment(spans, score, frame_logp, gaps, ali), or None where no alignment
    exists (fewer frames than tokens + adjacent repeats, as before). ValueError: everything
    align_long checks, a gap position outside [1, len(y) - 1], gap_penalty NaN or > 0: all before
    the device is touched. One avsr_ctc_align_gaps launch."""
    y = _transcript(e2e, y)
    pen = _gap_penalty(gap_penalty)
    flags = gap_flags(len(y), free_start, free_end, gaps)
    T = _frames(logits, lse)
    eng = e2e.engine()
    dev = eng.device
    lab, llen = _labels(y, dev)
    gap = torch.zeros(1, lab.shape[1] + 1, dtype=torch.uint8)
    gap[0, :len(y) + 1] = torch.tensor(flags, dtype=torch.uint8)
    filler = logits[:, :eng.V].amax(1).float() - lse
    ali, score, feas = ops.ctc_align_gaps(logits, 1, T, eng.V, lab, llen, torch.tensor([T], dtype=torch.int32).to(dev),
                                          lse, gap.to(dev), filler, pen, blank=e2e.blank)
    if not int(feas.item()):
        return None
    ingap = ali[0] == ops.CTC_ALIGN_GAP
    tok = torch.where(ingap, torch.full_like(ali[0], e2e.blank), ali[0])
    flp = torch.where(ingap, filler + pen, logits.gather(1, tok.view(T, 1).long()).view(T).float() - lse)
    ali = ali[0].cpu().numpy()
    return PartialAlignment(align.token_spans(tok.cpu().numpy(), e2e.blank), float(score.item()), flp.cpu().numpy(),
                            gap_runs(ali), ali)


def uncovered(alignment):
    """the stretches of the recording that a PartialAlignment left to its gaps, as (start, end)
    frame tuples in order: what a caller may want to transcribe (decode_stream on those frames)"""
    return [(int(a), int(b)) for a, b in alignment.gaps]


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
    the word's mean frame_logp (calibration unmeasured: module docstring). No tokens: [].

    An alignment with a `gaps` attribute (PartialAlignment: runs [start, end) of frames that the
    transcript does not cover) additionally: every pause that contains a gap run is a cut from
    the start, whatever max_frames; and a run's extent stays out of gap frames, lo >= the end of the
    last gap run at or before start_a and hi <= the start of the first gap run at or after end_b
    (instead of 0 and T at the recording's ends). With gaps == [] the result is that of the same
    spans as a LongAlignment. score / worst are as above: word frames are never gap frames. A gap
    run INSIDE a word (between two of its pieces, possible with gaps="all") stays in its clip."""
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
    holes = [(int(a), int(b)) for a, b in getattr(alignment, "gaps", ())]
    floor = [max([b for _, b in holes if b <= start[i]], default=0) for i in range(n)]
    ceil = [min([a for a, _ in holes if a >= end[i]], default=T) for i in range(n)]
    forced = [i for i in range(n - 1) if any(a >= end[i] and b <= start[i + 1] for a, b in holes)]

    def extent(a, b):
        lo = max(cut[a - 1] if a > 0 else 0, start[a] - margin, floor[a])
        hi = min(cut[b] if b < n - 1 else T, end[b] + margin, ceil[b])
        return lo, hi

    firsts = [0] + [i + 1 for i in forced]
    runs, todo = [], list(zip(firsts, [i for i in forced] + [n - 1]))[::-1]
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

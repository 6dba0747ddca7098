"""Plain CPU references of the beam-search kernels (decode_softmax.hip, dec_attn.hip,
ctc_prefix.hip, beam.hip), written from the contract in include/avsr_hip.h: numpy / torch fp64 or exact integer logic, no project kernel and nothing of
avsr_amd.ops. Shared by tests/test_gpu_decode_kernels.py (kernel by kernel),
tests/test_gpu_decode_scripted.py (the real step sequence on a table decoder) and
tests/test_decode_scripted_cases.py (what the scripted cases cover, from the reference alone)."""
import functools
import math

import numpy as np
import torch

from oracle import decode_oracle as DO

LOGZERO = -10000000000.0
D_END = float(np.log(1 * np.exp(-10)))
NEG_INF = float("-inf")


# ------------------------------------------------------------------------------ top-k
def topk_ref(x, K):
    """ids of the K largest entries per row: value descending, then index ascending (-inf
    entries count as the smallest value, in index order). x: (rows, V) numpy."""
    x = np.asarray(x)
    idx = np.arange(x.shape[1])
    return np.stack([np.lexsort((idx, -row.astype(np.float64)))[:K] for row in x])


# ------------------------------------------------------------------------------ attention
def attn_ref(q, keys, vals, H, scale=0.125):
    """softmax(scale * q k^T) v of one query (H*64,) over its key / value rows (L, H*64),
    fp64. Pass the stored values (for bf16 storage: the rounded ones)."""
    q = q.double().view(H, 64)
    k = keys.double().view(-1, H, 64)
    v = vals.double().view(-1, H, 64)
    s = torch.einsum("hd,jhd->hj", q, k) * scale
    return torch.einsum("hj,jhd->hd", torch.softmax(s, -1), v).reshape(H * 64)


def attn_close(o, ref, bf16):
    """fp32: 1e-5 absolute. bf16 storage: 2^-8 |ref| + 1e-4 (one bf16 rounding of the output is
    2^-9 relative, doubled for an fp32 result on the other side of a rounding boundary)."""
    err = (o.double().cpu() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-4 if bf16 else torch.full_like(ref, 1e-5)
    return bool((err <= bound).all()), float((err - bound).max())


# ------------------------------------------------------------------------------ beam_select
def beam_select_ref(dec, ids, psi, s_prev, score, *, beam, blank, eos, w_dec, w_ctc, seg=None):
    """avsr_beam_select restated: the full weighted[n][V] matrix per segment, its top `beam` by
    value descending then flat index ascending. numpy inputs; dec (n, V), ids (n, P), psi
    (n, P + 1), s_prev / score (n,). The matrix is built in fp32 in the documented order
    (w_dec*dec + w_ctc*(psi - s_prev) + score), which is exact for the quantised inputs the tests
    use; LOGZERO-class entries (|x| ~ 1e9..1e10, one fp32 ulp >= 64) absorb the small terms.
    Returns a dict of the seven outputs, [nseg * beam]."""
    n, V = dec.shape
    P = ids.shape[1]
    f = np.float32
    segs = [0, n] if seg is None else list(seg)
    out = {k: [] for k in ("prev", "tok", "col", "score", "dec", "ctc", "s")}
    for u in range(len(segs) - 1):
        r0, r1 = segs[u], segs[u + 1]
        if all(score[h] == NEG_INF for h in range(r0, r1)):      # the documented filler
            for _ in range(beam):
                for k, v in (("prev", r0), ("tok", eos), ("col", P - 1), ("score", NEG_INF), ("dec", 0.0),
                             ("ctc", 0.0), ("s", 0.0)):
                    out[k].append(v)
            continue
        full_psi = np.full((r1 - r0, V), f(LOGZERO), dtype=f)
        for h in range(r0, r1):
            for c in range(P - 1, -1, -1):                       # (first column wins on a repeat)
                full_psi[h - r0, ids[h, c]] = psi[h, c]
            full_psi[h - r0, eos] = psi[h, P]
            full_psi[h - r0, blank] = f(LOGZERO)
        sp, sc = s_prev[r0:r1, None].astype(f), score[r0:r1, None].astype(f)
        weighted = (f(w_dec) * dec[r0:r1].astype(f) + f(w_ctc) * (full_psi - sp)).astype(f) + sc
        weighted[score[r0:r1] == NEG_INF] = NEG_INF
        flat = weighted.reshape(-1)
        order = np.lexsort((np.arange(flat.size), -flat.astype(np.float64)))[:beam]
        for fl in order.tolist():
            hl, tok = fl // V, fl % V
            h = r0 + hl
            hit = np.nonzero(ids[h] == tok)[0]
            out["prev"].append(h)
            out["tok"].append(tok)
            out["col"].append(int(hit[0]) if len(hit) else P - 1)
            out["score"].append(float(flat[fl]))
            out["dec"].append(float(dec[h, tok]))
            out["ctc"].append(float(f(full_psi[hl, tok]) - f(s_prev[h])))
            out["s"].append(float(full_psi[hl, tok]))
    return out


# ------------------------------------------------------------------------------ beam_post
class BeamPostRef:
    """avsr_beam_post restated from include/avsr_hip.h and the search it replaces
    (batch_beam_search.py:262-349, beam_search.py:330-372, e2e_asr_common.py:18-48): U x beam
    rows, Python floats for the double sums, lists of ended (length, score) per utterance for the
    end detection."""

    def __init__(self, U, beam, P, maxlen, eos, sos, end_detect, steps):
        R = U * beam
        self.U, self.beam, self.P, self.R, self.eos, self.end_detect = U, beam, P, R, eos, end_detect
        self.maxlen = list(maxlen)
        self.Lmax = steps + 1
        self.pos = 0
        self.tok = [sos] * R
        self.score = [0.0 if r % beam == 0 else NEG_INF for r in range(R)]
        self.sdec, self.sctc, self.s_prev = [0.0] * R, [0.0] * R, [0.0] * R
        self.src = [0] * (2 * R)
        z = lambda v: [[v] * R for _ in range(steps)]
        self.bp_prev, self.bp_tok, self.end_flag = z(0), z(0), z(0)
        self.end_score, self.end_dec, self.end_ctc = z(0.0), z(0.0), z(0.0)
        self.best_len = [[NEG_INF] * (self.Lmax + 3) for _ in range(U)]
        self.best_end = [NEG_INF] * U
        self.done = [0] * (U + 1)
        self.ended = [[] for _ in range(U)]          # (len(yseq), score) of every ended hypothesis
        self.events = set()

    def step(self, sel):
        """sel: dict prev/tok/col (ints), score/dec/ctc/s (fp32 values as Python floats), [R]"""
        R, beam, P, pos = self.R, self.beam, self.P, self.pos
        od, oc = list(self.sdec), list(self.sctc)
        was_done = list(self.done[:self.U])
        live = [False] * self.U
        for r in range(R):
            u = r // beam
            if was_done[u]:                          # finished before this step: stays dead
                self.score[r] = NEG_INF
                self.src[r], self.src[R + r] = r, r * P
                self.bp_prev[pos][r], self.bp_tok[pos][r], self.end_flag[pos][r] = r, self.eos, 0
                self.events.add("dead_after_done")
                continue
            h, t, sc = sel["prev"][r], sel["tok"][r], sel["score"][r]
            nd, nc = od[h] + sel["dec"][r], oc[h] + sel["ctc"][r]
            forced = pos == self.maxlen[u] - 1       # eos appended to every hypothesis at the last step
            e = 2 if forced else (1 if t == self.eos else 0)
            self.bp_prev[pos][r], self.bp_tok[pos][r], self.end_flag[pos][r] = h, t, e
            if e:
                self.end_score[pos][r], self.end_dec[pos][r], self.end_ctc[pos][r] = sc, nd, nc
                self.ended[u].append((pos + 2 + (1 if e == 2 else 0), sc))      # sos + pos+1 tokens (+ forced eos)
                self.events.add("eos" if e == 1 else ("forced_on_eos" if t == self.eos else "forced"))
            else:
                live[u] = True
            self.tok[r] = t
            self.score[r] = NEG_INF if e else sc
            self.sdec[r], self.sctc[r], self.s_prev[r] = nd, nc, sel["s"][r]
            self.src[r], self.src[R + r] = h, h * P + sel["col"][r]
        for u in range(self.U):
            if was_done[u]:
                continue
            for ln, sc in self.ended[u]:
                if ln < self.Lmax + 3:
                    self.best_len[u][ln] = max(self.best_len[u][ln], sc)
                self.best_end[u] = max(self.best_end[u], sc)
            det = False
            if self.end_detect and self.ended[u]:    # e2e_asr_common.end_detect, M = 3
                best = max(s for _, s in self.ended[u])
                count = 0
                for m in range(3):
                    same = [s for ln, s in self.ended[u] if ln == pos - m]
                    if same and max(same) - best < D_END:
                        count += 1
                det = count == 3
                if det:
                    self.events.add("end_detect")
            if not live[u] and not det and pos < self.maxlen[u] - 1:
                self.events.add("no_live_row")
            if det or not live[u] or pos >= self.maxlen[u] - 1:
                self.done[u] = 1
                for k in range(beam):
                    self.score[u * beam + k] = NEG_INF
        self.done[self.U] = sum(self.done[:self.U])
        self.pos = pos + 1


# ------------------------------------------------------------------------------ scripted search
def scripted_case(seed, U, beam, w, T_lo=6, T_hi=20, V=32, kind="random", Ts=None):
    """inputs of one scripted search: Ts, table (U, Tmax, V, V) fp32 decoder logits (row: step,
    last token), ctc (U, Tmax, V) fp32 CTC log-probs (frames past T_u hold other values: they
    must not be read)"""
    g = torch.Generator().manual_seed(seed)
    if Ts is None:
        Ts = [int(t) for t in torch.randint(T_lo, T_hi + 1, (U,), generator=g)]
    Tm = max(Ts)
    if kind == "random":
        table = torch.randn(U, Tm, V, V, generator=g) * 2
        ctc = torch.randn(U, Tm, V, generator=g) * 3
    else:                                            # end detection: an early eos far above the rest
        table = torch.randn(U, Tm, V, V, generator=g) * 0.5
        table[:, 0, :, V - 1] += 6
        table[:, 1:, :, V - 1] += 1
        ctc = torch.randn(U, Tm, V, generator=g) * 3
        if kind == "end_detect":
            ctc[:, :, 0] += 6
    return dict(seed=seed, U=U, beam=beam, w=w, Ts=Ts, V=V, table=table.float(),
                ctc=torch.log_softmax(ctc.float(), -1), kind=kind, maxlenratio=0.0)


def scripted_search_ref(table, ctc_logp, beam_size, ctc_weight, maxlenratio=0.0):
    """oracle.decode_oracle.beam_search with decoder_one_step replaced by the table lookup
    (row = (step, last token) -> logits, log-softmax in fp64), everything in fp64. table
    (steps, V, V), ctc_logp (T, V). Returns (ended hypotheses best first, info) with info =
    the smallest gap between successive entries of the top beam + 1 weighted scores over all
    steps relative to its skip threshold, and which events the search met."""
    table, ctc_logp = table.double(), ctc_logp.double()
    T, V = ctc_logp.shape
    sos = eos = V - 1
    blank = 0
    w_dec, w_ctc = 1.0 - ctc_weight, ctc_weight
    use_dec, use_ctc = w_dec != 0.0, w_ctc != 0.0
    pre_beam = int(1.5 * beam_size)
    maxlen = T if maxlenratio == 0 else (-int(maxlenratio) if maxlenratio < 0 else max(1, int(maxlenratio * T)))
    running = [DO.Hyp([sos], 0.0, {k: 0.0 for k, u in (("decoder", use_dec), ("ctc", use_ctc)) if u}, None, 0.0)]
    ended = []
    info = dict(margin=math.inf, eos_early=False, forced=False, unscored=False, end_detect=False, steps=0)
    for i in range(maxlen):
        n = len(running)
        info["steps"] = i + 1
        weighted = torch.zeros(n, V, dtype=torch.float64)
        if use_dec:
            dec = torch.log_softmax(table[i][[h.yseq[-1] for h in running]], -1)
            weighted = weighted + w_dec * dec
        if use_ctc:
            ids = torch.topk(dec, pre_beam, dim=-1)[1] if use_dec else torch.arange(V).expand(n, V)
            states = [None if h.ctc_r is None else (h.ctc_r, h.ctc_s) for h in running]
            ctc_sc, r_new, log_psi = DO.ctc_prefix_scores(ctc_logp, [h.yseq for h in running], states, ids, blank, eos)
            weighted = weighted + w_ctc * ctc_sc
        weighted = weighted + torch.tensor([h.score for h in running], dtype=weighted.dtype).unsqueeze(1)
        vals, top = weighted.view(-1).topk(min(beam_size + 1, n * V))
        for a, b in zip(vals[:-1].tolist(), vals[1:].tolist()):
            # two scores that each err by the project's 1e-4 * |score| + 1e-4 could swap
            info["margin"] = min(info["margin"], (a - b) / (2 * (1e-4 * max(abs(a), abs(b)) + 1e-4)))
        best = []
        for flat in top[:beam_size].tolist():
            p, tok = flat // V, flat % V
            h = running[p]
            sc = {}
            if use_dec:
                sc["decoder"] = h.scores["decoder"] + float(dec[p, tok])
            if not use_ctc:
                best.append(DO.Hyp(h.yseq + [tok], float(weighted[p, tok]), sc, None, 0.0))
                continue
            pos = (ids[p] == tok).nonzero()
            if not len(pos):
                info["unscored"] = True
            col = int(pos[0, 0]) if len(pos) else ids.shape[1] - 1      # scoring_idmap -1 => index -1
            sc["ctc"] = h.scores["ctc"] + float(ctc_sc[p, tok])
            best.append(DO.Hyp(h.yseq + [tok], float(weighted[p, tok]), sc, r_new[:, :, p, col].clone(),
                               float(log_psi[p, tok])))
        if i == maxlen - 1:
            info["forced"] = True
            best = [DO.Hyp(h.yseq + [eos], h.score, h.scores, h.ctc_r, h.ctc_s) for h in best]
        elif any(h.yseq[-1] == eos for h in best):
            info["eos_early"] = True
        running = []
        for h in best:
            (ended if h.yseq[-1] == eos else running).append(h)
        if maxlenratio == 0.0 and DO.end_detect(ended, i):
            info["end_detect"] = True
            break
        if not running:
            break
    return sorted(ended, key=lambda h: h.score, reverse=True), info


# The scripted batches: (seed, beam, ctc_weight, kind), each U = 4 utterances = 4 cases (one
# reference search each): 15 random batches (60 cases: T 6..20, every beam 1/3/5 x ctc_weight
# 0/0.1/0.5/1) and 6 batches built for end detection (T = 16, beam 3). The seeds are the first ones
# from 1001 on whose batch has no skipped case (at most one at beam 5), for the constructed
# batches also at least two cases that fire end detection (not asked at ctc_weight 1) -- found from the fp64
# reference alone, as tests/test_decode_scripted_cases.py re-checks.
SCRIPTED_U = 4
SCRIPTED_BATCHES = [
    (1001, 1, 0.0, "random"), (1002, 1, 0.1, "random"), (1003, 1, 0.5, "random"), (1004, 1, 1.0, "random"),
    (1005, 3, 0.0, "random"), (1006, 3, 0.1, "random"), (1010, 3, 0.5, "random"), (1012, 3, 1.0, "random"),
    (1014, 5, 0.0, "random"), (1017, 5, 0.1, "random"), (1021, 5, 0.5, "random"), (1022, 5, 1.0, "random"),
    (1025, 3, 0.1, "random"), (1026, 5, 0.5, "random"), (1027, 5, 1.0, "random"),
    (1048, 3, 0.1, "end_detect"), (1051, 3, 0.5, "end_detect"), (1053, 3, 1.0, "end_detect"),
    (1059, 3, 0.5, "end_detect"), (1072, 3, 0.0, "end_detect_w0"), (1073, 3, 0.0, "end_detect_w0")]
MAX_SKIP_SHARE = 0.10


@functools.lru_cache(maxsize=None)
def scripted_reference(batch):
    """(inputs, per utterance (hyps, info, skipped)) of one scripted batch. A case is skipped when
    its reference's own smallest top-(beam + 1) gap is under 2 * (1e-4 * |score| + 1e-4): decided
    here, from the fp64 reference alone."""
    seed, beam, w, kind = batch
    T = dict(T_lo=6, T_hi=20) if kind == "random" else dict(T_lo=16, T_hi=16)
    c = scripted_case(seed, SCRIPTED_U, beam, w, kind=kind, **T)
    refs = []
    for u in range(c["U"]):
        hyps, info = scripted_search_ref(c["table"][u, :c["Ts"][u]], c["ctc"][u, :c["Ts"][u]], beam, w)
        refs.append((hyps, info, info["margin"] < 1.0))
    return c, refs


def long_case():
    """one utterance of 250 frames at ctc_weight = 1, maxlenratio 0.05 (12 steps): the full
    vocabulary goes through the prefix kernel in chunks of 64 ids, 250 * 67 * 4 B > 64 KiB, so the
    non-LDS kernel runs inside a search"""
    c = scripted_case(3002, 1, 3, 1.0, Ts=[250], V=32)      # (3001: top scores closer than the skip rule allows)
    c["maxlenratio"] = 0.05
    return c

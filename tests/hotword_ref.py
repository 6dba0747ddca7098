"""Plain CPU references of hot-word biasing in the beam search, written from the rule stated in
avsr_amd/hotwords.py and include/avsr_hip.h (avsr_hotword_step, the bonus fields of
avsr_beam_select / avsr_beam_post): a dict prefix tree and its scorer walk, the per-step kernel's
outputs, beam_select with the bonus, and the fp64 search of tests/decode_ref.py with biasing.
Nothing of avsr_amd.ops. Shared by tests/test_hotword_host.py (no GPU),
tests/test_gpu_hotword_kernel.py and tests/test_gpu_hotword_search.py."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import decode_oracle as DO
from tests import decode_ref as R

C = 8                     # continuation columns per row
LOGZERO = R.LOGZERO
NEG_INF = R.NEG_INF


# ------------------------------------------------------------------------------ prefix tree
class Trie:
    """prefix tree over phrases as dicts. Nodes are numbered as avsr_amd.hotwords documents:
    depth-first, the children of a node in ascending token order (= creation order when the sorted
    phrases are inserted one after another); node 0 is the root."""

    def __init__(self, phrases, eos):
        self.eos = eos
        self.kids, self.parent, self.terminal, self.depth = [{}], [-1], [False], [0]
        for p in sorted({tuple(p) for p in phrases}):
            n = 0
            for t in p:
                if t not in self.kids[n]:
                    self.kids[n][t] = len(self.kids)
                    self.kids.append({})
                    self.parent.append(n)
                    self.terminal.append(False)
                    self.depth.append(self.depth[n] + 1)
                n = self.kids[n][t]
            self.terminal[n] = True

    def pend(self, n):
        """depth(n) minus the depth of the nearest terminal ancestor-or-self (0 without one)"""
        a = n
        while a > 0 and not self.terminal[a]:
            a = self.parent[a]
        return self.depth[n] - (self.depth[a] if a > 0 else 0)

    def _land(self, m):
        return 0 if self.terminal[m] and not self.kids[m] else m

    def step(self, n, v, cancel=True):
        """(k, next node, what happened) of extending a hypothesis at node n with token v; the
        bonus is beta * k. cancel=False: a variant that never takes a bonus back (tests only)"""
        if v in self.kids[n]:
            m = self.kids[n][v]
            return 1, self._land(m), {"match"} | ({"complete"} if self.terminal[m] else set())
        k = -self.pend(n) if cancel else 0
        what = {"cancel"} if self.pend(n) else set()
        if v != self.eos and v in self.kids[0]:
            m = self.kids[0][v]
            return k + 1, self._land(m), what | {"match"} | ({"complete"} if self.terminal[m] else set())
        return k, 0, what

    def walk(self, tokens, node=0):
        ks = []
        for v in tokens:
            k, node, _ = self.step(node, v)
            ks.append(k)
        return ks, node


# the phrase sets of the tests (V = 12: blank 0, tokens 1 .. 10, eos 11)
SET_A = [[3], [4, 5, 6], [4, 5, 7]]                 # a single-token phrase; two phrases sharing a prefix
SET_B = [[2, 3], [2, 3, 4, 5], [6, 6, 8]]           # a proper prefix of another; a repeated token
SET_FAN = [[1, t] for t in range(2, 10)]            # node "1" has exactly 8 children
SETS = {"A": SET_A, "B": SET_B, "AB": SET_A + SET_B}


# ------------------------------------------------------------------------------ per-step kernel
def candidates_ref(trie, node, pre, blank=0):
    """the row's P + C candidate ids: the pre-beam, then child j of a non-root node in token order at
    column P + j unless the pre-beam holds it; blank elsewhere"""
    extra = [blank] * C
    if node != 0:
        for j, t in enumerate(sorted(trie.kids[node])[:C]):
            if t not in pre:
                extra[j] = t
    return list(pre) + extra


def hotword_step_ref(trie, nodes, ids_pre, beta, blank=0):
    """avsr_hotword_step restated: ids (R, P + C) int32, bonus (R, P + C + 1) fp32 = beta * float(k)
    as one fp32 product, next (R, P + C + 1) int32; the last column is eos. A blank column is an
    eos-like mismatch (no child, no restart)."""
    ids_pre = np.asarray(ids_pre)
    Rn, P = ids_pre.shape
    ids = np.zeros((Rn, P + C), np.int32)
    bonus = np.zeros((Rn, P + C + 1), np.float32)
    nxt = np.zeros((Rn, P + C + 1), np.int32)
    for r in range(Rn):
        n = int(nodes[r])
        ids[r] = candidates_ref(trie, n, [int(t) for t in ids_pre[r]], blank)
        for c, v in enumerate(list(ids[r]) + [trie.eos]):
            k, nx, _ = trie.step(n, int(v))
            bonus[r, c] = np.float32(beta) * np.float32(k)
            nxt[r, c] = nx
    return ids, bonus, nxt


# ------------------------------------------------------------------------------ beam_select
def beam_select_bonus_ref(dec, ids, psi, s_prev, score, bonus, nxt, *, beam, blank, eos, w_dec, w_ctc, seg=None,
                          lm=None, lm_next=None, w_lm=0.0, w_len=0.0):
    """decode_ref.beam_select_ref with the hot-word bonus: weighted = w_dec*dec + w_ctc*(psi - s_prev)
    + bonus + score, the fp32 sums in this order; the bonus of token v of row h is bonus[h][c], c its
    first column in ids[h], or P (the eos column) for eos, blank and every token outside ids[h].
    With an n-gram LM (lm / lm_next (n, P + 1)) or a length bonus (w_len != 0) the sum takes the
    order include/avsr_hip.h states: w_dec*dec + w_len + w_lm*lm + w_ctc*(psi - s_prev) [+ bonus] +
    score; the LM column of v is its first column in ids[h], P for eos, and none for blank and every
    token outside ids[h]: an LM term of 0 and a successor of -1. bonus None: no bonus term.
    Returns the seven outputs of beam_select_ref plus "bonus" and "next" (with bonus) and "lm" and
    "lm_next" (with lm)."""
    n, V = dec.shape
    P = ids.shape[1]
    f = np.float32
    segs = [0, n] if seg is None else list(seg)
    keys = ("prev", "tok", "col", "score", "dec", "ctc", "s") + (("bonus", "next") if bonus is not None else ()) + \
        (("lm", "lm_next") if lm is not None else ())
    filler = dict(prev=None, tok=eos, col=P - 1, score=NEG_INF, dec=0.0, ctc=0.0, s=0.0, bonus=0.0, next=0, lm=0.0,
                  lm_next=-1)
    out = {k: [] for k in keys}
    for u in range(len(segs) - 1):
        r0, r1 = segs[u], segs[u + 1]
        if all(score[h] == NEG_INF for h in range(r0, r1)):
            for _ in range(beam):
                for k in keys:
                    out[k].append(r0 if k == "prev" else filler[k])
            continue
        full_psi = np.full((r1 - r0, V), f(LOGZERO), dtype=f)
        bcol = np.full((r1 - r0, V), P, dtype=np.int64)
        lcol = np.full((r1 - r0, V), -1, dtype=np.int64)
        for h in range(r0, r1):
            for c in range(P - 1, -1, -1):                       # (first column wins on a repeat)
                full_psi[h - r0, ids[h, c]] = psi[h, c]
                if ids[h, c] not in (eos, blank):
                    bcol[h - r0, ids[h, c]] = lcol[h - r0, ids[h, c]] = c
            full_psi[h - r0, eos] = psi[h, P]
            full_psi[h - r0, blank] = f(LOGZERO)
            lcol[h - r0, eos] = P
        sp, sc = s_prev[r0:r1, None].astype(f), score[r0:r1, None].astype(f)
        weighted = f(w_dec) * dec[r0:r1].astype(f)
        if lm is not None or w_len != 0.0:
            weighted = (weighted + f(w_len)).astype(f)
            if lm is not None:
                full_lm = np.stack([np.where(lcol[h - r0] >= 0, lm[h].astype(f)[lcol[h - r0]], f(0.0))
                                    for h in range(r0, r1)]).astype(f)
                weighted = (weighted + f(w_lm) * full_lm).astype(f)
        weighted = (weighted + f(w_ctc) * (full_psi - sp)).astype(f)
        if bonus is not None:
            full_b = np.stack([bonus[h].astype(f)[bcol[h - r0]] for h in range(r0, r1)])
            weighted = (weighted + full_b).astype(f)
        weighted = weighted + sc
        weighted[score[r0:r1] == NEG_INF] = NEG_INF
        flat = weighted.reshape(-1)
        order = np.lexsort((np.arange(flat.size), -flat.astype(np.float64)))[:beam]
        for fl in order.tolist():
            hl, tok = fl // V, fl % V
            h = r0 + hl
            hit = np.nonzero(ids[h] == tok)[0]
            lc = int(lcol[hl, tok])
            row = dict(prev=h, tok=tok, col=int(hit[0]) if len(hit) else P - 1, score=float(flat[fl]),
                       dec=float(dec[h, tok]), ctc=float(f(full_psi[hl, tok]) - f(s_prev[h])), s=float(full_psi[hl, tok]))
            if bonus is not None:
                row.update(bonus=float(full_b[hl, tok]), next=int(nxt[h, bcol[hl, tok]]))
            if lm is not None:
                row.update(lm=float(lm[h, lc]) if lc >= 0 else 0.0, lm_next=int(lm_next[h, lc]) if lc >= 0 else -1)
            for k in keys:
                out[k].append(row[k])
    return out


# ------------------------------------------------------------------------------ the search
@dataclass
class HHyp(DO.Hyp):
    node: int = 0
    tags: frozenset = frozenset()         # what its hot-word walk met: extra / complete / cancel


def hotword_search_ref(table, ctc_logp, beam_size, ctc_weight, phrases, beta, cancel=True):
    """decode_ref.scripted_search_ref (the joint search, maxlenratio 0) with hot-word biasing, all
    in fp64. phrases None: the plain search (the same code with no bonus and no extra candidate).
    Every row's candidates are its pre-beam, eos and the continuations of its node; a candidate's
    bonus is beta * k of the tree step, every other token's the cancellation alone; selection on
    w_dec*dec + w_ctc*ctc + bonus + score; the bonus sum is scores["hotword"]; the eos a length
    limit appends is not scored. Returns (ended hypotheses best first, info): info["margin"] as in
    scripted_search_ref (smallest gap within the top beam + 1 over twice the tolerance)."""
    table, ctc_logp = table.double(), ctc_logp.double()
    T, V = ctc_logp.shape
    sos = eos = V - 1
    blank = 0
    w_dec, w_ctc = 1.0 - ctc_weight, ctc_weight
    P = int(1.5 * beam_size)
    trie = None if phrases is None else Trie(phrases, eos)
    s0 = {"decoder": 0.0, "ctc": 0.0, **({} if trie is None else {"hotword": 0.0})}
    running = [HHyp([sos], 0.0, s0, None, 0.0)]
    ended = []
    info = dict(margin=math.inf, steps=0)
    for i in range(T):
        n = len(running)
        info["steps"] = i + 1
        dec = torch.log_softmax(table[i][[h.yseq[-1] for h in running]], -1)
        pre = torch.topk(dec, P, dim=-1)[1]
        if trie is None:
            ids = pre
        else:
            ids = torch.tensor([candidates_ref(trie, h.node, pre[p].tolist(), blank) for p, h in enumerate(running)])
        states = [None if h.ctc_r is None else (h.ctc_r, h.ctc_s) for h in running]
        ctc_sc, r_new, log_psi = DO.ctc_prefix_scores(ctc_logp, [h.yseq for h in running], states, ids, blank, eos)
        weighted = w_dec * dec + w_ctc * ctc_sc
        steps = None
        if trie is not None:
            steps = []                                   # per row: {token: (k, next, what)} of its candidates
            bonus = torch.zeros(n, V, dtype=torch.float64)
            for p, h in enumerate(running):
                other = trie.step(h.node, eos, cancel)   # a token outside the candidates: like eos
                row = {v: other for v in range(V)}
                for v in ids[p].tolist() + [eos]:
                    if v != blank:
                        row[v] = trie.step(h.node, v, cancel)
                steps.append(row)
                bonus[p] = torch.tensor([beta * float(row[v][0]) for v in range(V)], dtype=torch.float64)
            weighted = weighted + bonus
        weighted = weighted + torch.tensor([h.score for h in running], dtype=torch.float64).unsqueeze(1)
        vals, top = weighted.view(-1).topk(min(beam_size + 1, n * V))
        for a, b in zip(vals[:-1].tolist(), vals[1:].tolist()):
            info["margin"] = min(info["margin"], (a - b) / (2 * (1e-4 * max(abs(a), abs(b)) + 1e-4)))
        best = []
        for flat in top[:beam_size].tolist():
            p, tok = flat // V, flat % V
            h = running[p]
            sc = {"decoder": h.scores["decoder"] + float(dec[p, tok]), "ctc": h.scores["ctc"] + float(ctc_sc[p, tok])}
            pos = (ids[p] == tok).nonzero()
            col = int(pos[0, 0]) if len(pos) else ids.shape[1] - 1
            node, tags = 0, h.tags
            if trie is not None:
                k, node, what = steps[p][tok]
                sc["hotword"] = h.scores["hotword"] + beta * float(k)
                tags = tags | (what & {"complete", "cancel"})
                if tok not in (eos, blank) and tok in ids[p, P:].tolist():
                    tags = tags | {"extra"}
            best.append(HHyp(h.yseq + [tok], float(weighted[p, tok]), sc, r_new[:, :, p, col].clone(),
                             float(log_psi[p, tok]), node, frozenset(tags)))
        if i == T - 1:
            best = [HHyp(h.yseq + [eos], h.score, h.scores, h.ctc_r, h.ctc_s, h.node, h.tags) for h in best]
        running = []
        for h in best:
            (ended if h.yseq[-1] == eos else running).append(h)
        if DO.end_detect(ended, i) or not running:
            break
    return sorted(ended, key=lambda h: h.score, reverse=True), info


# The search cases: (seed, beam, ctc_weight, phrase set, beta), each a batch of 3 utterances of
# T = 6, 9, 7 frames over V = 12. Every beam x ctc_weight x beta once per phrase-set rotation; the
# seeds are the first from 2001 on whose three reference searches keep every top-(beam + 1) gap at
# twice the tolerance or more (no case is skipped), found from the fp64 reference alone;
# tests/test_hotword_host.py re-checks that and what the cases cover.
SEARCH_TS = [6, 9, 7]
SEARCH_V = 12
SEARCH_CASES = [
    (2001, 3, 0.1, "A", 0.75), (2002, 3, 0.1, "B", 3.0), (2003, 3, 0.3, "AB", 0.75), (2004, 3, 0.3, "A", 3.0),
    (2006, 5, 0.1, "B", 0.75), (2007, 5, 0.1, "AB", 3.0), (2008, 5, 0.3, "A", 0.75), (2009, 5, 0.3, "B", 3.0)]
# the cases whose plain search (no phrase list) is compared with the reference too: its gaps hold as well
CLEARED_CASES = [SEARCH_CASES[1], SEARCH_CASES[5]]


@functools.lru_cache(maxsize=None)
def search_reference(case):
    """(inputs, [(biased hyps, info, plain hyps, no-cancel hyps, plain info)] per utterance) of one case"""
    seed, beam, w, name, beta = case
    c = R.scripted_case(seed, len(SEARCH_TS), beam, w, V=SEARCH_V, Ts=SEARCH_TS)
    c["phrases"], c["beta"] = SETS[name], beta
    refs = []
    for u, T in enumerate(c["Ts"]):
        tab, ctc = c["table"][u, :T], c["ctc"][u, :T]
        hyps, info = hotword_search_ref(tab, ctc, beam, w, c["phrases"], beta)
        plain, plain_info = hotword_search_ref(tab, ctc, beam, w, None, beta)
        nocancel, _ = hotword_search_ref(tab, ctc, beam, w, c["phrases"], beta, cancel=False)
        refs.append((hyps, info, plain, nocancel, plain_info))
    return c, refs

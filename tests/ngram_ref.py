"""Plain CPU references of n-gram LM shallow fusion, written from the rule stated in
avsr_amd/ngram_lm.py and include/avsr_hip.h (avsr_ngram_step, avsr_ngram_score_seqs, the LM and
length-bonus fields of avsr_beam_select / avsr_beam_post): a dict-based backoff model in fp64, the
per-step kernel's outputs, and the fp64 search of tests/decode_ref.py / tests/hotword_ref.py with
the LM and length terms in the reference's summation order (batch_beam_search.py:222-245: full
scorers in the order of its scorer dict, then partial scorers, then the running score). Nothing of
avsr_amd.ngram_lm or avsr_amd.ops. Shared by tests/test_ngram_host.py (no GPU),
tests/test_gpu_ngram_kernel.py and tests/test_gpu_ngram_search.py."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import decode_oracle as DO
from tests import decode_ref as R
from tests import hotword_ref as H

V = 12                    # blank 0, tokens 1 .. 10, sos = eos = 11
SOS = EOS = V - 1
BLANK = 0
TOKENS = list(range(1, 11))


# ------------------------------------------------------------------------------ the model
class RefLM:
    """entries = {(context tuple, token): (logp, backoff)}, natural log, fp64 throughout. A state
    is the context tuple itself."""

    def __init__(self, order, entries, unk_logp, sos=SOS, eos=EOS):
        self.order, self.unk, self.sos, self.eos = order, float(unk_logp), sos, eos
        self.entries = {(tuple(c), int(v)): (float(p), float(b)) for (c, v), (p, b) in entries.items()
                        if len(c) + 1 <= order}
        seeds = [c for (c, _) in self.entries]
        seeds += [c + (v,) for (c, v), (_, b) in self.entries.items() if b != 0.0 and len(c) + 1 <= order - 1]
        if order > 1:
            seeds.append((sos,))
        self.contexts = {()} | set(seeds)
        for c in self.contexts:                          # an n-gram needs its prefix, as in ARPA files
            assert len(c) == 0 or c == (sos,) or (c[:-1], c[-1]) in self.entries, c

    def backoff(self, ctx):
        return self.entries.get((ctx[:-1], ctx[-1]), (0.0, 0.0))[1] if ctx else 0.0

    def state(self, history):
        """the longest suffix of the history (sos first; at most order - 1 tokens) that is a context"""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        for i in range(len(h) + 1):
            if h[i:] in self.contexts:
                return h[i:]

    def score(self, ctx, v):
        """(score, successor context, (order of the entry hit or 0 for unk_logp, contexts left))"""
        nxt = self.state(ctx + (v,))
        acc, left = 0.0, 0
        while True:
            if (ctx, v) in self.entries:
                return acc + self.entries[(ctx, v)][0], nxt, (len(ctx) + 1, left)
            if not ctx:
                return acc + self.unk, nxt, (0, left)
            acc += self.backoff(ctx)
            ctx = ctx[1:]
            left += 1

    def score_tokens(self, tokens):
        """per-token scores of tokens + [eos] from the <s> state"""
        ctx, out = self.state((self.sos,)), []
        for v in list(tokens) + [self.eos]:
            s, ctx, _ = self.score(ctx, int(v))
            out.append(s)
        return out


def _q(x):
    """values on a grid of 1/64: exact in fp32, and so are short sums of them"""
    return round(float(x) * 64.0) / 64.0


def make_table(seed, order=4, contexts=(10, 60, 250), kids=(6, 4, 4)):
    """a seeded table over the 10 tokens and eos: unigrams for tokens 1 .. 9 and eos (token 10 has
    none: it scores unk_logp), then per level k = 2 .. order `contexts[k - 2]` contexts of k - 1 tokens
    (over tokens 1 .. 9; the first may be sos) with `kids[k - 2]` entries each, plus the entry every
    context needs to be listed itself; higher orders score higher, three in ten entries carry no
    backoff"""
    rng = np.random.RandomState(seed)
    ent = {}
    for v in TOKENS[:-1] + [EOS]:
        ent[((), v)] = (_q(rng.uniform(-4.0, -2.0)), _q(rng.uniform(-1.0, -0.1)))
    for k in range(2, order + 1):
        seen = set()
        while len(seen) < contexts[k - 2]:
            c = tuple(int(t) for t in rng.choice(TOKENS[:-1], k - 1))
            if rng.rand() < 0.15:
                c = (SOS,) + c[1:]
            seen.add(c)
        for c in sorted(seen):
            for v in rng.choice(TOKENS + [EOS], kids[k - 2], replace=False):
                bo = 0.0 if rng.rand() < 0.3 else _q(rng.uniform(-0.8, -0.05))
                ent[(c, int(v))] = (_q(rng.uniform(-1.5, -0.1)), bo)
    for c in sorted({c for c, _ in ent}, key=lambda c: (-len(c), c)):      # longest first: prefixes of prefixes
        while len(c) > 1 and (c[:-1], c[-1]) not in ent:
            ent[(c[:-1], c[-1])] = (_q(rng.uniform(-1.5, -0.1)), _q(rng.uniform(-0.8, -0.05)))
            c = c[:-1]
    return ent


UNK = -3.0
SEARCH_TABLE = make_table(41)
# the kernel tests' table, by hand: node (1,) has 9 entries, (2,) one, (3,) none (a context only through
# the backoff of its unigram); (1, 2) and (1, 2, 3) give a full-depth chain; contexts beginning with sos
KERNEL_TABLE = {
    **{((), v): (_q(-2.0 - 0.25 * v), _q(-0.5 - 0.0625 * v) if v in (1, 2, 3, 5, EOS) else 0.0) for v in TOKENS[:-1] + [EOS]},
    **{((1,), v): (_q(-1.0 - 0.125 * v), _q(-0.25) if v in (2, 4) else 0.0) for v in range(1, 10)},
    ((2,), 5): (-0.75, 0.0),
    ((SOS,), 1): (-0.5, -0.125), ((SOS,), 4): (-1.25, 0.0),
    ((1, 2), 3): (-0.375, -0.5), ((1, 2), 9): (-0.625, 0.0), ((1, 4), 4): (-0.875, 0.0),
    ((SOS, 1), 2): (-0.25, -0.375), ((5,), 1): (-0.9375, -0.1875), ((5, 1), 2): (-0.3125, 0.0),
    ((1, 2, 3), 4): (-0.125, 0.0), ((1, 2, 3), EOS): (-0.0625, 0.0), ((SOS, 1, 2), 3): (-0.1875, 0.0),
}


def table_lm(table, order, unk=UNK):
    return RefLM(order, table, unk)


# ------------------------------------------------------------------------------ per-step kernel
def ngram_step_ref(lm, states, ids):
    """avsr_ngram_step restated: score (R, P + 1) fp64 and the successor context per column, for
    rows at the context tuples `states`; the last column is eos; a blank column gets 0 and the row's
    own state"""
    ids = np.asarray(ids)
    Rn, P = ids.shape
    score = np.zeros((Rn, P + 1))
    nxt = [[None] * (P + 1) for _ in range(Rn)]
    for r in range(Rn):
        for c, v in enumerate(list(ids[r]) + [lm.eos]):
            if c < P and v == BLANK:
                score[r, c], nxt[r][c] = 0.0, states[r]
            else:
                score[r, c], nxt[r][c], _ = lm.score(states[r], int(v))
    return score, nxt


# ------------------------------------------------------------------------------ the search
@dataclass
class LHyp(DO.Hyp):
    node: int = 0                         # hot-word tree node
    ctx: tuple = ()                       # LM state
    tags: frozenset = frozenset()         # ("order", k) of every LM entry hit, ("left", n), "extra", "unscored"


def lm_search_ref(table, ctc_logp, beam_size, ctc_weight, lm=None, w_lm=0.0, w_len=0.0, phrases=None, beta=0.0):
    """decode_ref.scripted_search_ref (the joint search, maxlenratio 0) with an LM scorer, a length
    bonus and optionally hot words, all in fp64: weighted = w_dec*dec + w_len*1 + w_lm*lm + w_ctc*ctc
    [+ hot-word bonus] + score, in this order. As in the reference every token of every row gets its
    LM score (the device gives a token outside a row's candidates 0 there; such a token sits at
    w_ctc * LOGZERO and is never selected: a selected one is tagged "unscored"). scores["lm"] is the
    unweighted sum, scores["length_bonus"] the number of scored tokens; the eos a length limit appends
    is not scored. Returns (ended hypotheses best first, info): info["margin"] as in
    scripted_search_ref, info["ended_by"] "end_detect" / "limit" / "no_running"."""
    table, ctc_logp = table.double(), ctc_logp.double()
    T, Vn = ctc_logp.shape
    sos = eos = Vn - 1
    w_dec, w_ctc = 1.0 - ctc_weight, ctc_weight
    P = int(1.5 * beam_size)
    trie = None if phrases is None else H.Trie(phrases, eos)
    s0 = {"decoder": 0.0, "ctc": 0.0}
    if lm is not None:
        s0["lm"] = 0.0
    if w_len != 0.0:
        s0["length_bonus"] = 0.0
    if trie is not None:
        s0["hotword"] = 0.0
    running = [LHyp([sos], 0.0, s0, None, 0.0, 0, lm.state((sos,)) if lm is not None else ())]
    ended = []
    info = dict(margin=math.inf, steps=0, ended_by="limit")
    for i in range(T):
        n = len(running)
        info["steps"] = i + 1
        dec = torch.log_softmax(table[i][[h.yseq[-1] for h in running]], -1)
        pre = torch.topk(dec, P, dim=-1)[1]
        if trie is None:
            ids = pre
        else:
            ids = torch.tensor([H.candidates_ref(trie, h.node, pre[p].tolist(), BLANK) for p, h in enumerate(running)])
        states = [None if h.ctc_r is None else (h.ctc_r, h.ctc_s) for h in running]
        ctc_sc, r_new, log_psi = DO.ctc_prefix_scores(ctc_logp, [h.yseq for h in running], states, ids, BLANK, eos)
        weighted = w_dec * dec
        if w_len != 0.0:
            weighted = weighted + w_len * torch.ones(n, Vn, dtype=torch.float64)
        lms = None
        if lm is not None:
            lms = [[lm.score(h.ctx, v) for v in range(Vn)] for h in running]
            weighted = weighted + w_lm * torch.tensor([[s for s, _, _ in row] for row in lms], dtype=torch.float64)
        weighted = weighted + w_ctc * ctc_sc
        steps = None
        if trie is not None:
            steps = []
            bonus = torch.zeros(n, Vn, dtype=torch.float64)
            for p, h in enumerate(running):
                other = trie.step(h.node, eos)
                row = {v: other for v in range(Vn)}
                for v in ids[p].tolist() + [eos]:
                    if v != BLANK:
                        row[v] = trie.step(h.node, v)
                steps.append(row)
                bonus[p] = torch.tensor([beta * float(row[v][0]) for v in range(Vn)], dtype=torch.float64)
            weighted = weighted + bonus
        weighted = weighted + torch.tensor([h.score for h in running], dtype=torch.float64).unsqueeze(1)
        vals, top = weighted.view(-1).topk(min(beam_size + 1, n * Vn))
        for a, b in zip(vals[:-1].tolist(), vals[1:].tolist()):
            info["margin"] = min(info["margin"], (a - b) / (2 * (1e-4 * max(abs(a), abs(b)) + 1e-4)))
        best = []
        for flat in top[:beam_size].tolist():
            p, tok = flat // Vn, flat % Vn
            h = running[p]
            sc = {"decoder": h.scores["decoder"] + float(dec[p, tok]), "ctc": h.scores["ctc"] + float(ctc_sc[p, tok])}
            pos = (ids[p] == tok).nonzero()
            col = int(pos[0, 0]) if len(pos) else ids.shape[1] - 1
            node, ctx, tags = 0, (), h.tags
            if tok != eos and (tok == BLANK or not len(pos)):
                tags = tags | {"unscored"}
            if lm is not None:
                s, ctx, (order_hit, left) = lms[p][tok]
                sc["lm"] = h.scores["lm"] + s
                tags = tags | {("order", order_hit), ("left", left)}
            if w_len != 0.0:
                sc["length_bonus"] = h.scores["length_bonus"] + 1.0
            if trie is not None:
                k, node, _ = steps[p][tok]
                sc["hotword"] = h.scores["hotword"] + beta * float(k)
                if tok not in (eos, BLANK) and tok in ids[p, P:].tolist():
                    tags = tags | {"extra"}
            best.append(LHyp(h.yseq + [tok], float(weighted[p, tok]), sc, r_new[:, :, p, col].clone(),
                             float(log_psi[p, tok]), node, ctx, frozenset(tags)))
        if i == T - 1:
            best = [LHyp(h.yseq + [eos], h.score, h.scores, h.ctc_r, h.ctc_s, h.node, h.ctx, h.tags) for h in best]
        running = []
        for h in best:
            (ended if h.yseq[-1] == eos else running).append(h)
        if DO.end_detect(ended, i):
            info["ended_by"] = "end_detect"
            break
        if not running:
            info["ended_by"] = "limit" if i == T - 1 else "no_running"
            break
    return sorted(ended, key=lambda h: h.score, reverse=True), info


# The search cases: (seed, beam, ctc_weight, kind, Ts, LM order or None, w_lm, w_len, phrase set or
# None, beta), each a batch of 3 utterances over V = 12 (decode_ref.scripted_case of that kind). The
# LM is SEARCH_TABLE cut to the order. Per row (beam 1 / 3 / 5; LM alone; length bonus alone; both;
# both with hot words) the seed is the first from 4001 on whose three reference searches, and the
# three without LM, keep every top-(beam + 1) gap at twice the tolerance or more and show what the
# row is there for (CASE_PURPOSE; tests/test_ngram_host.py re-checks both), found from the fp64
# reference alone. No case is skipped.
_T3 = (6, 9, 7)
SEARCH_CASES = [
    (4058, 1, 0.3, "random", _T3, 4, 1.5, 0.0, None, 0.0),
    (4001, 3, 0.1, "random", _T3, 4, 0.8, 0.0, None, 0.0),
    (4001, 5, 0.3, "random", _T3, 3, 0.5, 0.0, None, 0.0),
    (4001, 3, 0.3, "random", _T3, None, 0.0, -2.0, None, 0.0),
    (4016, 5, 0.1, "end_detect", (12, 10, 11), 2, 0.5, 0.5, None, 0.0),
    (4013, 3, 0.1, "random", _T3, 4, 0.7, 0.3, "AB", 1.5),
]
CASE_PURPOSE = [
    "beam 1, LM alone: the LM changes a best hypothesis; a winning path hits unk_logp and leaves all 3 context levels",
    "beam 3, LM alone: the LM changes a best hypothesis; winning paths use entries of orders 2, 3 and 4",
    "beam 5, order-3 LM alone: the LM changes a best hypothesis; a winning path backs off two levels",
    "length bonus alone (negative): the best hypothesis gets shorter",
    "LM and length bonus, eos-heavy tables: every utterance stops by end detection, with LM terms in all sums",
    "LM, length bonus and hot words: a winning path takes a hot-word continuation column, which the LM scored",
]


def case_id(c):
    return f"s{c[0]}-b{c[1]}-w{c[2]:g}-lm{c[5]}x{c[6]:g}-len{c[7]:g}-{c[8]}"


@functools.lru_cache(maxsize=None)
def search_reference(case):
    """(inputs, [(hyps, info, plain hyps, plain info)] per utterance) of one case; plain = the same
    search without LM, length bonus and hot words"""
    seed, beam, w, kind, Ts, order, w_lm, w_len, pset, beta = case
    c = R.scripted_case(seed, len(Ts), beam, w, V=V, Ts=list(Ts), kind=kind)
    lm = None if order is None else table_lm(SEARCH_TABLE, order)
    c.update(lm=lm, order=order, w_lm=w_lm, w_len=w_len, phrases=None if pset is None else H.SETS[pset], beta=beta)
    refs = []
    for u, T in enumerate(c["Ts"]):
        tab, ctc = c["table"][u, :T], c["ctc"][u, :T]
        hyps, info = lm_search_ref(tab, ctc, beam, w, lm, w_lm, w_len, c["phrases"], beta)
        plain, plain_info = lm_search_ref(tab, ctc, beam, w)
        refs.append((hyps, info, plain, plain_info))
    return c, refs


# ------------------------------------------------------------------------------ the reference's own search
def load_lm_fixture():
    """tests/golden/avsr_lm.npz (tests/golden/make_golden_lm.py: the reference's BatchBeamSearch
    with a LengthBonus and an n-gram scorer on the tiny model): dict of order, unk, entries (the
    table, as RefLM / NgramLM.from_table take it), settings [(lm_weight, length_bonus)], and
    runs[(setting, clip)] = dict(steps, hyps [dict(yseq, score, scores)] best first)"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avsr_lm.npz"))
    entries = {}
    for row, p, b in zip(z["tab_tok"].tolist(), z["tab_logp"].tolist(), z["tab_bo"].tolist()):
        entries[(tuple(t for t in row[:-1] if t >= 0), row[-1])] = (p, b)
    fx = dict(order=int(z["order"]), unk=float(z["unk"]), entries=entries,
              settings=[tuple(s) for s in z["settings"].tolist()], runs={})
    for s in range(len(fx["settings"])):
        for c in range(2):
            key = f"lm{s}_{c}"
            ends = np.cumsum(z[key + "_len"]).tolist()
            hyps = []
            for i, (a, b) in enumerate(zip([0] + ends[:-1], ends)):
                scores = {n: float(z[f"{key}_{n}"][i]) for n in ("decoder", "ctc", "lm", "length_bonus") if f"{key}_{n}" in z}
                hyps.append(dict(yseq=z[key + "_yseq"][a:b].tolist(), score=float(z[key + "_score"][i]), scores=scores))
            fx["runs"][(s, c)] = dict(steps=int(z[key + "_steps"]), hyps=hyps)
    return fx

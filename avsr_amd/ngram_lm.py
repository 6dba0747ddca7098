"""Token-level backoff n-gram language model for shallow fusion: the host side.

An `NgramLM` (order 1 to 6) over the model's token ids is compiled into flat int32 / fp32 arrays,
which the searches upload once and two kernels walk (csrc/ngram.hip, avsr_hip.h avsr_ngram_step for
the joint search's step, avsr_ngram_score_seqs for the two-pass decoder).

The scoring rule (the kernels, `NgramLM.step` here and tests/ngram_ref.py state the same rule).
The model is a set of entries (context, token) -> (logp, backoff), natural log, the context a tuple
of 0 to order-1 token ids, oldest first, which may begin with sos (ARPA's <s>). The backoff of the
entry (c, v) is the backoff weight of the context c + (v,). The contexts of the model are the
context of every entry, every c + (v,) of at most order-1 tokens whose entry has a non-zero
backoff, (sos,) when order > 1, and the empty context. As ARPA requires, an n-gram may only be
listed when its prefix is: every context c + (v,) other than (sos,) must be an entry (c, v) itself
(ValueError otherwise), which is what makes the successor below a function of the entry hit.
  state    of a hypothesis: the longest suffix of its history (sos included, at most order-1
           tokens) that is a context. A fresh hypothesis stands at the state of (sos,).
  score(state, v): acc = 0. If (context, v) is an entry, the result is acc + logp. Otherwise
           acc += the context's backoff (0 if it has none), the context loses its oldest token,
           and the lookup repeats. At the empty context a token without an entry gets unk_logp.
  next     the successor state is the longest suffix of context + (v,) that is a context: fixed
           per entry (and per token at the empty context), so it is precomputed here.
The rule is that of ARPA / SRILM / KenLM backoff models. No normalisation is required or checked.
<s> is never predicted and </s> (eos) never part of a context, so a model whose sos and eos share
one id (this project's) keeps them apart: that id inside a context is <s>, as a token it is </s>.

Compiled form (node 0 is the empty context, `start` the node of (sos,); the nodes are the contexts
and those of their suffixes that are none, which have no entries and no backoff and are only passed
through on a fail link, never a state):
  per node   child_off [nodes + 1], backoff [nodes], fail [nodes] (the node of the context without
             its oldest token), ctx_tok [nodes] (that oldest token; host only)
  per entry  with a non-empty context, token-sorted inside its node's span
             [child_off[n], child_off[n + 1]): tok, logp, next
  dense      uni_logp [V], uni_next [V]: the empty context needs no search
  lm_hi      an upper bound on any score: max(0, max logp) + (order - 1) * max(0, max backoff)
Values go through fp64 and are stored as fp32. The compile step is numpy over whole n-gram levels
(sort, unique, searchsorted; no Python loop over entries); `from_arpa` splits the text line by line
in Python. Compiling 1e6 entries from arrays takes about a second; the load time of an
ARPA file of millions of entries, text parsing included, has not been measured.
"""
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_ORDER = 6
_LN10 = math.log(10.0)


class NgramLM:
    """a compiled backoff n-gram model (see the module docstring); build one with `from_arpa` or
    `from_table`"""

    ARRAYS = ("child_off", "backoff", "fail", "tok", "logp", "next", "uni_logp", "uni_next")

    def __init__(self, order, grams, sos, eos, n_vocab, unk_logp):
        """grams: {k: (tokens int [n, k], logp fp64 [n], backoff fp64 [n])} for k = 1 .. order, a
        k-gram being the entry (tokens[:k-1], tokens[k-1]); a NaN unigram logp means "no unigram" """
        order, V = int(order), int(n_vocab)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"order {order} outside [1, {MAX_ORDER}]")
        if V < 2 or not (0 <= int(sos) < V and 0 <= int(eos) < V):
            raise ValueError(f"sos {sos} / eos {eos} outside a vocabulary of {V}")
        if unk_logp is not None and not math.isfinite(float(unk_logp)):
            raise ValueError(f"unk_logp {unk_logp!r} is not finite")
        self.order, self.n_vocab, self.sos, self.eos = order, V, int(sos), int(eos)
        self.unk_logp = None if unk_logp is None else float(unk_logp)
        self._compile({k: (np.asarray(t, np.int64).reshape(-1, k), np.asarray(p, np.float64).reshape(-1),
                           np.asarray(b, np.float64).reshape(-1)) for k, (t, p, b) in grams.items()})

    # --------------------------------------------------------------------------- constructors
    @classmethod
    def from_table(cls, order, entries: Dict[Tuple[Tuple[int, ...], int], Tuple[float, float]], sos, eos, n_vocab,
                   unk_logp):
        """entries = {(context tuple, token): (logp, backoff)} in natural log (see the module
        docstring). The logp of an entry predicting sos is never read unless sos == eos."""
        if unk_logp is None:
            raise ValueError("from_table needs unk_logp")
        rows = {}
        for (ctx, v), (lp, bo) in entries.items():
            k = len(ctx) + 1
            if k > int(order):
                raise ValueError(f"entry {(ctx, v)} is longer than the order {order}")
            if not (math.isfinite(float(lp)) and math.isfinite(float(bo))):
                raise ValueError(f"entry {(ctx, v)}: logp / backoff must be finite")
            rows.setdefault(k, []).append((tuple(ctx) + (v,), float(lp), float(bo)))
        grams = {}
        for k in range(1, int(order) + 1):
            r = rows.get(k, [])
            grams[k] = (np.array([t for t, _, _ in r], np.int64).reshape(-1, k), np.array([p for _, p, _ in r]),
                        np.array([b for _, _, b in r]))
        return cls(order, grams, sos, eos, n_vocab, unk_logp)

    @classmethod
    def from_arpa(cls, path_or_text, token_list: Sequence[str], sos, eos, unk_logp=None):
        """standard ARPA text (a path, or the text itself): log10 values, \\data\\, \\N-grams:
        sections with an optional backoff column, \\end\\. Words are the strings of token_list; <s>
        is the start context only (its unigram gives a backoff, its -99 is ignored), </s> is eos.
        ValueError for a word that is neither in token_list nor <s> / </s> / <unk>, and for a
        vocabulary token (other than blank, id 0) without a unigram when neither unk_logp nor an
        <unk> unigram gives it a score."""
        text = path_or_text
        if "\n" not in text and "\\data\\" not in text:     # a path (FileNotFoundError if there is no such file)
            with open(text, "r", encoding="utf-8") as f:
                text = f.read()
        ids = {w: i for i, w in enumerate(token_list)}
        ids["<s>"], ids["</s>"] = int(sos), int(eos)
        V = len(token_list)
        counts, rows, k, unk, s_bo = {}, {}, 0, None, 0.0
        for ln, line in enumerate(text.splitlines(), 1):
            line = line.strip()
            if not line or line == "\\data\\":
                continue
            if line == "\\end\\":
                break
            if line.startswith("ngram ") and k == 0:
                n, c = line[6:].split("=")
                counts[int(n)] = int(c)
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                k = int(line[1:-7])
                rows[k] = ([], [], [])
                continue
            f = line.split()
            if k == 0 or len(f) not in (k + 1, k + 2):
                raise ValueError(f"ARPA line {ln}: {line!r}")
            lp, words = float(f[0]) * _LN10, f[1:k + 1]
            bo = float(f[k + 1]) * _LN10 if len(f) == k + 2 else 0.0
            if k == 1 and words[0] == "<unk>":
                unk = lp
                continue
            if k == 1 and words[0] == "<s>":            # the start context: a backoff, no prediction
                s_bo = bo
                continue
            try:
                t = [ids[w] for w in words]
            except KeyError as e:
                raise ValueError(f"ARPA line {ln}: word {e.args[0]!r} is not in the token list") from None
            if "<unk>" in words or "<s>" in words[1:] or "</s>" in words[:-1]:
                raise ValueError(f"ARPA line {ln}: <unk> / <s> / </s> out of place in {words}")
            rows[k][0].append(t)
            rows[k][1].append(lp)
            rows[k][2].append(bo)
        order = max(rows) if rows else 0
        if not 1 <= order <= MAX_ORDER or sorted(rows) != list(range(1, order + 1)):
            raise ValueError(f"ARPA sections {sorted(rows)}: need 1 .. N with N <= {MAX_ORDER}")
        grams = {j: (np.array(t, np.int64).reshape(-1, j), np.array(p, np.float64), np.array(b, np.float64))
                 for j, (t, p, b) in rows.items()}
        # <s>'s backoff belongs to the id sos at the unigram level: on the </s> row when the model
        # shares the id, else on a row of its own without a logp
        t1, p1, b1 = grams[1]
        hit = np.nonzero(t1[:, 0] == int(sos))[0]
        if len(hit):
            b1[hit[0]] = s_bo
        else:
            t1, p1, b1 = np.vstack([t1, [[int(sos)]]]), np.append(p1, np.nan), np.append(b1, s_bo)
        grams[1] = (t1, p1, b1)
        lm = cls(order, grams, sos, eos, V, unk if unk_logp is None else unk_logp)
        lm.arpa_counts = counts
        return lm

    # --------------------------------------------------------------------------- compile
    def _walk_levels(self, seqs, exact=False):
        """node of the longest suffix of each row of seqs (n, m) that is a context (levels built so
        far); with exact, also whether the whole row is one"""
        n, m = seqs.shape
        cur = np.zeros(n, np.int64)
        alive = np.ones(n, bool)
        for j in range(1, m + 1):
            if j > len(self._level_keys):
                alive[:] = False
                break
            keys = self._level_keys[j - 1]
            key = cur * self.n_vocab + seqs[:, m - j]
            idx = np.minimum(np.searchsorted(keys, key), max(len(keys) - 1, 0))
            found = alive & (keys[idx] == key) if len(keys) else np.zeros(n, bool)
            cur = np.where(found, self._level_base[j - 1] + idx, cur)
            alive = found
        return (cur, alive) if exact else self._canon[cur]

    def _compile(self, grams):
        order, V = self.order, self.n_vocab
        for k in range(1, order + 1):
            grams.setdefault(k, (np.zeros((0, k), np.int64), np.zeros(0), np.zeros(0)))
        for k, (t, p, b) in grams.items():
            if not 1 <= k <= order or not (len(t) == len(p) == len(b)):
                raise ValueError(f"{k}-grams: bad shapes for an order-{order} model")
            if t.size and (t.min() < 0 or t.max() >= V):
                raise ValueError(f"{k}-grams hold a token id outside [0, {V})")
        # the contexts, level by level (level j = contexts of j tokens): every suffix of a seed
        seeds = [grams[k][0][:, :k - 1] for k in range(2, order + 1)]
        seeds += [grams[k][0][grams[k][2] != 0.0] for k in range(1, order)]
        if order > 1:
            seeds.append(np.array([[self.sos]], np.int64))
        seeds = [s for s in seeds if len(s)]
        self._level_keys, self._level_base, self._canon = [], [], None
        cur = [np.zeros(len(s), np.int64) for s in seeds]
        nodes, fail, ctx_tok = 1, [np.zeros(1, np.int64)], [np.full(1, -1, np.int64)]
        for j in range(1, order):
            part = [(i, cur[i] * V + s[:, s.shape[1] - j]) for i, s in enumerate(seeds) if s.shape[1] >= j]
            keys = np.unique(np.concatenate([k for _, k in part])) if part else np.zeros(0, np.int64)
            self._level_keys.append(keys)
            self._level_base.append(nodes)
            for i, k in part:
                cur[i] = nodes + np.searchsorted(keys, k)
            fail.append(keys // V)
            ctx_tok.append(keys % V)
            nodes += len(keys)
        fail, ctx_tok = np.concatenate(fail), np.concatenate(ctx_tok)
        real = np.zeros(nodes, bool)                     # a context, not only the suffix of one
        real[0] = True
        for c in cur:
            real[c] = True
        backoff, listed = np.zeros(nodes, np.float64), np.zeros(nodes, bool)
        for k in range(1, order):
            t, _, b = grams[k]
            if len(t):
                node, is_ctx = self._walk_levels(t, exact=True)
                backoff[node[is_ctx]] = b[is_ctx]
                listed[node[is_ctx]] = True
        listed[0] = True
        if order > 1:
            listed[self._walk_levels(np.array([[self.sos]], np.int64), exact=True)[0]] = True
        self.fail, self.ctx_tok = fail, ctx_tok
        if np.any(real & ~listed):
            bad = self.context(int(np.nonzero(real & ~listed)[0][0]))
            raise ValueError(f"the context {bad} of an entry is not listed as an n-gram itself (an n-gram needs its "
                             f"prefix, as in ARPA files)")
        canon = np.arange(nodes)
        for j, base in enumerate(self._level_base):     # a level's fail links point into the levels before it
            lv = slice(base, base + len(self._level_keys[j]))
            canon[lv] = np.where(real[lv], canon[lv], canon[fail[lv]])
        self._canon = canon
        # the entries below the unigram level, sorted by (node, token)
        cid, tok, logp, nxt = [], [], [], []
        for k in range(2, order + 1):
            t, p, _ = grams[k]
            if len(t):
                cid.append(self._walk_levels(t[:, :k - 1]))
                tok.append(t[:, k - 1])
                logp.append(p)
                nxt.append(self._walk_levels(t[:, max(0, k - (order - 1)):]))
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)      # noqa: E731
        cid, tok, logp, nxt = cat(cid, np.int64), cat(tok, np.int64), cat(logp, np.float64), cat(nxt, np.int64)
        o = np.lexsort((tok, cid))
        cid, tok, logp, nxt = cid[o], tok[o], logp[o], nxt[o]
        if len(cid) > 1 and np.any((cid[1:] == cid[:-1]) & (tok[1:] == tok[:-1])):
            raise ValueError("an n-gram is listed twice")
        child_off = np.zeros(nodes + 1, np.int64)
        np.cumsum(np.bincount(cid, minlength=nodes), out=child_off[1:])
        # the unigram level, dense
        t1, p1, _ = grams[1]
        if len(np.unique(t1[:, 0])) != len(t1):
            raise ValueError("a unigram is listed twice")
        uni = np.full(V, np.nan)
        uni[t1[:, 0]] = p1
        never = np.zeros(V, bool)
        never[0] = True                                  # blank, and <s> where it has an id of its own
        never[self.sos] = self.sos != self.eos
        missing = np.isnan(uni)
        if np.any(missing & ~never) and self.unk_logp is None:
            raise ValueError(f"{int(np.sum(missing & ~never))} vocabulary tokens have no unigram (the first: id "
                             f"{int(np.nonzero(missing & ~never)[0][0])}) and there is neither <unk> nor unk_logp")
        uni[missing] = 0.0 if self.unk_logp is None else self.unk_logp
        uni_next = self._walk_levels(np.arange(V, dtype=np.int64).reshape(V, 1)) if order > 1 else np.zeros(V, np.int64)
        if not (np.all(np.isfinite(uni)) and np.all(np.isfinite(logp)) and np.all(np.isfinite(backoff))):
            raise ValueError("logp / backoff must be finite")
        if nodes >= 2 ** 31 or len(tok) >= 2 ** 31:
            raise ValueError("the model does not fit int32 indices")
        i32, f32 = np.int32, np.float32
        self.child_off, self.backoff, self.fail = child_off.astype(i32), backoff.astype(f32), fail.astype(i32)
        self.ctx_tok = ctx_tok.astype(i32)
        self.tok, self.logp, self.next = tok.astype(i32), logp.astype(f32), nxt.astype(i32)
        self.uni_logp, self.uni_next = uni.astype(f32), uni_next.astype(i32)
        self.start = int(self._walk_levels(np.array([[self.sos]], np.int64))[0]) if order > 1 else 0
        top = max(float(self.uni_logp.max()), float(self.logp.max()) if len(tok) else -math.inf)
        self.lm_hi = float(max(0.0, top) + (order - 1) * max(0.0, float(self.backoff.max())))

    # --------------------------------------------------------------------------- host walk
    @property
    def nodes(self) -> int:
        return int(self.backoff.shape[0])

    @property
    def entries(self) -> int:
        """entries below the unigram level (the unigram level is dense)"""
        return int(self.tok.shape[0])

    def context(self, node: int) -> Tuple[int, ...]:
        """the context tuple of a node, oldest token first"""
        out = []
        while node != 0:
            out.append(int(self.ctx_tok[node]))
            node = int(self.fail[node])
        return tuple(out)

    def state_of(self, history: Sequence[int]) -> int:
        """the state of a hypothesis with this history (sos first)"""
        h = [int(t) for t in history][-(self.order - 1):] if self.order > 1 else []
        return int(self._walk_levels(np.array([h], np.int64).reshape(1, len(h)))[0])

    def step(self, state: int, v: int) -> Tuple[float, int]:
        """(score, successor state) of token v at `state`, walking the compiled arrays as the
        kernels do, the sum in fp64"""
        n, acc = int(state), 0.0
        while n != 0:
            lo, end = int(self.child_off[n]), int(self.child_off[n + 1])
            i = lo + int(np.searchsorted(self.tok[lo:end], v))
            if i < end and int(self.tok[i]) == v:
                return acc + float(self.logp[i]), int(self.next[i])
            acc += float(self.backoff[n])
            n = int(self.fail[n])
        return acc + float(self.uni_logp[v]), int(self.uni_next[v])

    def score_tokens(self, tokens: Sequence[int]) -> List[float]:
        """per-token scores of [tokens..., eos] from the <s> state, in fp64 (len(tokens) + 1 values)"""
        state, out = self.start, []
        for v in [int(t) for t in tokens] + [self.eos]:
            if not 0 <= v < self.n_vocab:
                raise ValueError(f"token id {v} outside [0, {self.n_vocab})")
            s, state = self.step(state, v)
            out.append(s)
        return out


def check_fusion(lm, weight, length_bonus, n_vocab, sos, eos):
    """the argument rules of `set_lm`, shared by the joint search and the two-pass decoder:
    (lm or None, lm weight, length bonus) as they take effect. weight finite and >= 0, length_bonus
    finite, a non-zero weight needs an lm, an lm of weight 0 is dropped (as the reference drops a
    scorer of weight 0), and the lm's vocabulary size / sos / eos must be the search's (n_vocab None:
    not known to the search). ValueError otherwise."""
    weight, length_bonus = float(weight), float(length_bonus)
    if not math.isfinite(weight) or weight < 0.0:
        raise ValueError(f"lm weight must be finite and >= 0 (got {weight!r})")
    if not math.isfinite(length_bonus):
        raise ValueError(f"length_bonus must be finite (got {length_bonus!r})")
    if lm is None and weight != 0.0:
        raise ValueError("a non-zero lm weight needs an lm")
    if lm is not None and weight == 0.0:
        lm = None
    if lm is not None:
        want = (lm.n_vocab if n_vocab is None else int(n_vocab), sos, eos)
        if (lm.n_vocab, lm.sos, lm.eos) != want:
            raise ValueError(f"the LM's vocabulary / sos / eos {(lm.n_vocab, lm.sos, lm.eos)} are not the search's {want}")
    return lm, weight if lm is not None else 0.0, length_bonus


class FusionArrays:
    """the device form of a search's LM, uploaded once per device and LM"""

    def __init__(self):
        self._lm, self._dev = None, {}

    def get(self, lm, dev):
        from . import ops
        if lm is not self._lm:
            self._lm, self._dev = lm, {}
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = ops.ngram_arrays(lm, dev)
        return self._dev[key]

"""Hot-word (contextual) biasing for the device beam search: the host side.

A phrase list becomes a prefix tree in flat int32 arrays, which the search uploads once and its
per-step kernel (csrc/hotword.hip, avsr_hip.h avsr_hotword_step) walks: every live hypothesis
carries a tree node, a token that continues a phrase earns `bonus`, a token that leaves a started
phrase gives back what the unfinished part earned (a context graph with fail arcs to the root).

Semantics (the kernel, `HotwordTree.step` here and tests/hotword_ref.py state the same rule).
Node 0 is the root; `pend[n]` = depth(n) minus the depth of the nearest terminal ancestor-or-self
(0 when there is none): the bonus tokens of n not yet earned by a completed phrase. Extending a
hypothesis at node n with token v gives k (the bonus is bonus * float(k), one fp32 product) and
the next node:
  child(n, v) = m exists:   k = 1, next = m; a terminal m without children sends next to the root
  v == eos:                 k = -pend[n], next = root
  otherwise (mismatch):     k = -pend[n], then from the root: child(root, v) = m exists -> k += 1,
                            next = m (same terminal rule); else next = root
Phrases are lists of token ids; `encode` turns texts into them with the caller's tokenizer.
"""
from typing import Callable, Iterable, List, NamedTuple, Sequence, Tuple

import numpy as np

MAX_CHILDREN = 8          # continuation candidates per hypothesis row (avsr_hip.h AVSR_HOTWORD_C)
MAX_NODES = 65535


class HotwordTree(NamedTuple):
    """prefix tree over the phrases, nodes numbered in depth-first order with the children of a
    node in ascending token order (the order of the sorted phrase list). Children of node n are
    entries [child_off[n], child_off[n + 1]) of child_tok (ascending) / child_node."""
    child_off: np.ndarray     # int32 [nodes + 1]
    child_tok: np.ndarray     # int32 [nodes - 1]
    child_node: np.ndarray    # int32 [nodes - 1]
    pend: np.ndarray          # int32 [nodes]
    terminal: np.ndarray      # int32 [nodes] 0 / 1
    depth: np.ndarray         # int32 [nodes]
    eos: int

    @property
    def nodes(self) -> int:
        return int(self.pend.shape[0])

    @property
    def max_depth(self) -> int:
        return int(self.depth.max())

    def child(self, n: int, v: int) -> int:
        """child(n, v) or -1: binary search of the node's sorted span (what the kernel does)"""
        lo, hi = int(self.child_off[n]), int(self.child_off[n + 1])
        while lo < hi:
            mid = (lo + hi) // 2
            if int(self.child_tok[mid]) < v:
                lo = mid + 1
            else:
                hi = mid
        if lo < int(self.child_off[n + 1]) and int(self.child_tok[lo]) == v:
            return int(self.child_node[lo])
        return -1

    def _land(self, m: int) -> int:
        leaf = self.child_off[m] == self.child_off[m + 1]
        return 0 if self.terminal[m] and leaf else m

    def step(self, n: int, v: int) -> Tuple[int, int]:
        """(k, next node) of extending a hypothesis at node n with token v"""
        m = self.child(n, v)
        if m >= 0:
            return 1, self._land(m)
        k = -int(self.pend[n])
        if v == self.eos:
            return k, 0
        m = self.child(0, v)
        if m >= 0:
            return k + 1, self._land(m)
        return k, 0

    def walk(self, tokens: Sequence[int], node: int = 0) -> Tuple[List[int], int]:
        """the k of every token of a sequence (sos excluded) from `node`, and the node after it"""
        ks = []
        for v in tokens:
            k, node = self.step(node, int(v))
            ks.append(k)
        return ks, node


def build_tree(phrases: Iterable[Sequence[int]], eos: int, blank: int = 0, max_children: int = MAX_CHILDREN,
               max_nodes: int = MAX_NODES) -> HotwordTree:
    """the prefix tree of `phrases` (lists of token ids; duplicates merge). ValueError for an empty
    list or phrase, blank / eos / a negative id in a phrase, a non-root node with more than
    `max_children` children (the search offers at most that many continuations per row, and drops
    none silently) and more than `max_nodes` nodes."""
    ps = sorted({tuple(int(t) for t in p) for p in phrases})
    if not ps:
        raise ValueError("no phrases")
    for p in ps:
        if not p:
            raise ValueError("empty phrase")
        for t in p:
            if t == blank or t == eos or t < 0:
                raise ValueError(f"phrase {list(p)} contains blank ({blank}), eos ({eos}) or a negative id")
    kids, terminal, depth = [{}], [0], [0]                  # per node: {token: child}
    for p in ps:                                            # sorted: nodes come out in depth-first order
        n = 0
        for t in p:
            m = kids[n].get(t)
            if m is None:
                m = kids[n][t] = len(kids)
                kids.append({})
                terminal.append(0)
                depth.append(depth[n] + 1)
                if len(kids) > max_nodes:
                    raise ValueError(f"more than {max_nodes} tree nodes")
            n = m
        terminal[n] = 1
    N = len(kids)
    for n in range(1, N):
        if len(kids[n]) > max_children:
            raise ValueError(f"a phrase prefix of {depth[n]} tokens has {len(kids[n])} continuations: "
                             f"at most {max_children} per node below the root")
    off = np.zeros(N + 1, np.int32)
    tok, node = [], []
    pend = np.zeros(N, np.int32)
    for n in range(N):
        for t in sorted(kids[n]):
            m = kids[n][t]
            tok.append(t)
            node.append(m)
            pend[m] = 0 if terminal[m] else pend[n] + 1     # (parents precede their children)
        off[n + 1] = len(tok)
    return HotwordTree(off, np.asarray(tok, np.int32), np.asarray(node, np.int32), pend,
                       np.asarray(terminal, np.int32), np.asarray(depth, np.int32), int(eos))


def encode(texts: Iterable[str], tokenize: Callable[[str], Sequence[int]]) -> List[List[int]]:
    """phrases as token-id lists from texts, through the caller's tokenizer (typically the
    reference's TextTransform.tokenize: the tokenizer stays host Python, as everywhere here)"""
    out = []
    for t in texts:
        ids = tokenize(t)
        out.append([int(i) for i in (ids.tolist() if hasattr(ids, "tolist") else ids)])
    return out

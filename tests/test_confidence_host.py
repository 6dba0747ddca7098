"""Host side of the confidences (avsr_amd/confidence.py): the fp64 reference of
tests/confidence_ref.py against hand-worked cases, the word aggregation against
align.word_times, argument validation, and the C-ABI mirror of avsr_ctc_neighbors. No GPU and no
kernel call."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import align, confidence
from tests import confidence_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")


def _logp(rows):
    return torch.tensor(rows, dtype=torch.float64).log()


def test_reference_two_frames_by_hand():
    """T = 2, V = 3, y = (1,): the paths of label v over two frames are (v, v), (blank, v) and
    (v, blank); the deletion is the all-blank path"""
    p = [[0.5, 0.3, 0.2], [0.1, 0.6, 0.3]]
    sub, dele, base = R.neighbors(_logp(p), [1], 2)
    p1 = 0.3 * 0.6 + 0.5 * 0.6 + 0.3 * 0.1
    p2 = 0.2 * 0.3 + 0.5 * 0.3 + 0.2 * 0.1
    pd = 0.5 * 0.1
    assert sub.shape == (1, 3) and sub[0, 0].item() == NEG_INF
    assert sub[0, 1].item() == pytest.approx(math.log(p1), abs=1e-14) and base == pytest.approx(math.log(p1), abs=1e-14)
    assert sub[0, 2].item() == pytest.approx(math.log(p2), abs=1e-14)
    assert dele[0].item() == pytest.approx(math.log(pd), abs=1e-14)          # L = 1: the all-blank path
    (conf, alts), = R.posteriors(sub, dele, [1], k=4)
    z = p1 + p2 + pd
    assert conf == pytest.approx(p1 / z, abs=1e-14)
    assert [a[0] for a in alts] == [2, None]
    assert [a[1] for a in alts] == pytest.approx([p2 / z, pd / z], abs=1e-14)
    # eos = 2 takes that column out of the outcomes
    sub_e, _, _ = R.neighbors(_logp(p), [1], 2, eos=2)
    assert sub_e[0, 2].item() == NEG_INF
    (conf_e, alts_e), = R.posteriors(sub_e, dele, [1], k=4, eos=2)
    assert conf_e == pytest.approx(p1 / (p1 + pd), abs=1e-14) and [a[0] for a in alts_e] == [None]


def test_reference_infeasible_substitute_is_minus_inf():
    """T = 2, y = (1, 2): a substitute equal to its neighbour needs a blank between, a third frame"""
    p = [[0.5, 0.3, 0.2], [0.1, 0.6, 0.3]]
    sub, dele, base = R.neighbors(_logp(p), [1, 2], 2)
    assert base == pytest.approx(math.log(0.3 * 0.3), abs=1e-14)              # the one path (1, 2)
    assert sub[0, 2].item() == NEG_INF and sub[1, 1].item() == NEG_INF          # (2, 2) and (1, 1)
    assert sub[0, 1].item() == pytest.approx(base, abs=1e-14) and sub[1, 2].item() == pytest.approx(base, abs=1e-14)
    # the deletions are one-label sequences over two frames
    assert dele[0].item() == pytest.approx(math.log(0.2 * 0.3 + 0.5 * 0.3 + 0.2 * 0.1), abs=1e-14)
    assert dele[1].item() == pytest.approx(math.log(0.3 * 0.6 + 0.5 * 0.6 + 0.3 * 0.1), abs=1e-14)
    # an outcome without a path is no alternative
    (c0, a0), _ = R.posteriors(sub, dele, [1, 2], k=4)
    assert [a[0] for a in a0] == [None]


def test_alternative_order_ties():
    """best first, ties to the lower id, the deletion last among equals -- reference and module"""
    sub = torch.tensor([[NEG_INF, -1.0, -2.0, -2.0, -3.0, NEG_INF]], dtype=torch.float64)
    dele = torch.tensor([-2.0], dtype=torch.float64)
    (_, alts), = R.posteriors(sub, dele, [1], k=4)
    assert [a[0] for a in alts] == [2, 3, None, 4]
    (_, alts2), = R.posteriors(sub, dele, [1], k=2)
    assert [a[0] for a in alts2] == [2, 3]
    cands = [(4, -3.0), (None, -2.0), (3, -2.0), (2, -2.0), (5, NEG_INF)]
    assert confidence.rank_alternatives(cands, 4) == [(2, -2.0), (3, -2.0), (None, -2.0), (4, -3.0)]
    assert confidence.rank_alternatives(cands, 16) == [(2, -2.0), (3, -2.0), (None, -2.0), (4, -3.0)]


def test_joint_confidence():
    assert confidence.joint_confidence(math.log(0.5), math.log(0.25), 0.5) == pytest.approx(math.sqrt(0.125), abs=1e-15)
    assert confidence.joint_confidence(math.log(0.5), None, 0.0) == pytest.approx(0.5, abs=1e-15)
    assert confidence.joint_confidence(None, math.log(0.25), 1.0) == pytest.approx(0.25, abs=1e-15)


TOKENS = ["<blank>", "▁a", "b", "▁c", "d", "<eos>"]


def _tc(tok, j):
    return confidence.TokenConfidence(tok, None, None, j, [])


def test_word_confidences_zip_with_word_times():
    toks = [_tc(1, 0.9), _tc(2, 0.5), _tc(3, 0.8)]                              # "▁a", "b", "▁c"
    spans = [align.TokenSpan(1, 0, 3), align.TokenSpan(2, 4, 5), align.TokenSpan(3, 7, 9)]
    times = align.word_times(spans, TOKENS, frame_rate=25.0)
    assert times == [("ab", 0.0, 0.2), ("c", 0.28, 0.36)]                       # unchanged by the shared helper
    for agg, first in (("min", 0.5), ("prod", 0.45), ("mean", 0.7)):
        words = confidence.word_confidences(toks, TOKENS, agg=agg)
        assert [w for w, _ in words] == [w for w, _, _ in times]
        assert words[0][1] == pytest.approx(first, abs=1e-15) and words[1][1] == 0.8
        assert words[0][1] == pytest.approx(R.word_agg([0.9, 0.5], agg), abs=1e-15)
    assert confidence.word_confidences(toks, TOKENS) == confidence.word_confidences(toks, TOKENS, agg="min")
    # a first piece without the space mark still opens a word
    toks2 = [_tc(2, 0.4), _tc(4, 0.6), _tc(1, 0.7)]                             # "b", "d", "▁a"
    spans2 = [align.TokenSpan(2, 0, 1), align.TokenSpan(4, 1, 2), align.TokenSpan(1, 5, 6)]
    assert confidence.word_confidences(toks2, TOKENS, agg="min") == [("bd", 0.4), ("a", 0.7)]
    assert [w for w, _, _ in align.word_times(spans2, TOKENS)] == ["bd", "a"]
    assert confidence.word_confidences([], TOKENS) == [] and align.word_times([], TOKENS) == []
    with pytest.raises(ValueError):
        confidence.word_confidences(toks, TOKENS, agg="max")


V = 6
STUB = types.SimpleNamespace(sos=V - 1, eos=V - 1, blank=0,
                             engine=lambda: types.SimpleNamespace(device="cpu", V=V))


def test_validation():
    x = torch.zeros(4, 8)
    for bad in (dict(xs=[x, x], yseqs=[[1]]),                                   # length mismatch
                dict(xs=[x], yseqs=[[1, V]]), dict(xs=[x], yseqs=[[-1]]),       # ids outside [0, V)
                dict(xs=[x], yseqs=[[1, 0, 2]]),                                # blank inside y
                dict(xs=[x], yseqs=[[1, V - 1, 2]]),                            # eos inside y
                dict(xs=[x], yseqs=[[1]], ctc_weight=-0.01), dict(xs=[x], yseqs=[[1]], ctc_weight=1.01),
                dict(xs=[x], yseqs=[[1]], alternatives=-1), dict(xs=[x], yseqs=[[1]], alternatives=17)):
        with pytest.raises(ValueError):
            confidence.confidence_batch(STUB, **bad)
    assert confidence.confidence_batch(STUB, [], []) == []


def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        parts = decl.replace("*", " ").replace(",", " ").split()
        quals = [w for w in parts if w in ("const", "unsigned")]
        ctype = parts[len(quals)]
        for fname in parts[len(quals) + 1:]:
            fields.append((fname, "ptr" if ptr else ctype))
    return fields


def test_struct_mirror_matches_header():
    """field order, offsets and size of CtcNeighborsParams against the C layout of the header's
    struct; the entry point is declared, bound and exported"""
    fields = _header_struct("avsr_ctc_neighbors_params")
    assert [f for f, _ in fields] == [f for f, _ in L.CtcNeighborsParams._fields_]
    size = {"int": 4, "float": 4, "int64_t": 8, "ptr": 8}
    off = 0
    for (fname, ctype), (_, mirror) in zip(fields, L.CtcNeighborsParams._fields_):
        off = -(-off // size[ctype]) * size[ctype]
        assert getattr(L.CtcNeighborsParams, fname).offset == off and ctypes.sizeof(mirror) == size[ctype], fname
        off += size[ctype]
    assert ctypes.sizeof(L.CtcNeighborsParams) == -(-off // 8) * 8
    assert fields[-1][0] == "lz"
    assert "avsr_ctc_neighbors" in L.SYMBOLS and hasattr(L.load(), "avsr_ctc_neighbors")
    # the workspace macro and its Python twin
    from avsr_amd import ops
    src = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    assert "AVSR_CTC_NEIGHBORS_WS(B, T, Lmax)" in src
    assert ops.ctc_neighbors_ws(8, 375, 40) == (8 * 375 * 81 * 2 * 4 + 15) // 16 * 16
    assert ops.ctc_neighbors_ws(1, 1, 1) == 32

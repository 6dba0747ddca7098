"""Host side of hot-word biasing (avsr_amd/hotwords.py, the set / clear / refuse rules of the
searches) and, from the fp64 reference alone, what the GPU search cases of
tests/test_gpu_hotword_search.py cover. No GPU and no kernel call."""
import types

import numpy as np
import pytest

from avsr_amd import hotwords as HW
from avsr_amd.avhubert_avsr_model import get_beam_search_decoder, get_rescoring_decoder
from tests import decode_ref as R
from tests import hotword_ref as H

V = 12
EOS = V - 1
TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, V - 1)] + ["<eos>"]
STUB = types.SimpleNamespace(sos=EOS, eos=EOS, engine=lambda: types.SimpleNamespace(device="cpu"))


def _arrays(t):
    return {k: getattr(t, k).tolist() for k in ("child_off", "child_tok", "child_node", "pend", "terminal", "depth")}


# ------------------------------------------------------------------------------ tree arrays
def test_tree_single_token_phrase_and_shared_prefix():
    """SET_A = [3], [4 5 6], [4 5 7]: nodes 0 root, 1 "3" (terminal leaf), 2 "4", 3 "4 5",
    4 "4 5 6", 5 "4 5 7"; the two phrases share nodes 2 and 3"""
    t = HW.build_tree(H.SET_A, eos=EOS)
    assert _arrays(t) == dict(child_off=[0, 2, 2, 3, 5, 5, 5], child_tok=[3, 4, 5, 6, 7], child_node=[1, 2, 3, 4, 5],
                              pend=[0, 0, 1, 2, 0, 0], terminal=[0, 1, 0, 0, 1, 1], depth=[0, 1, 1, 2, 3, 3])
    assert t.nodes == 6 and t.max_depth == 3
    assert all(a.dtype == np.int32 for a in t[:6])


def test_tree_proper_prefix_and_repeated_token():
    """SET_B = [2 3], [2 3 4 5], [6 6 8]: node 2 "2 3" is terminal with a child, so pend restarts
    there (node 3 "2 3 4" has 1 pending, not 3); "6 6 8" repeats a token: nodes 5 "6", 6 "6 6"
    are distinct"""
    t = HW.build_tree(H.SET_B, eos=EOS)
    assert _arrays(t) == dict(child_off=[0, 2, 3, 4, 5, 5, 6, 7, 7], child_tok=[2, 6, 3, 4, 5, 6, 8],
                              child_node=[1, 5, 2, 3, 4, 6, 7], pend=[0, 1, 0, 1, 0, 1, 2, 0],
                              terminal=[0, 0, 1, 0, 1, 0, 0, 1], depth=[0, 1, 2, 3, 4, 1, 2, 3])


@pytest.mark.parametrize("name", ["A", "B", "AB", "FAN"])
def test_tree_agrees_with_the_dict_reference(name):
    """numbering, children, pend, terminal flags and the step of every (node, token) equal the
    reference prefix tree's"""
    phrases = H.SET_FAN if name == "FAN" else H.SETS[name]
    t, ref = HW.build_tree(phrases, eos=EOS), H.Trie(phrases, EOS)
    assert t.nodes == len(ref.kids)
    for n in range(t.nodes):
        lo, hi = t.child_off[n], t.child_off[n + 1]
        assert dict(zip(t.child_tok[lo:hi].tolist(), t.child_node[lo:hi].tolist())) == ref.kids[n]
        assert t.child_tok[lo:hi].tolist() == sorted(ref.kids[n])
        assert (t.pend[n], bool(t.terminal[n]), t.depth[n]) == (ref.pend(n), ref.terminal[n], ref.depth[n])
        for v in range(V):
            assert t.step(n, v) == ref.step(n, v)[:2], (n, v)


def test_duplicates_merge_and_any_order():
    a = HW.build_tree(H.SET_B, eos=EOS)
    b = HW.build_tree([[6, 6, 8], (2, 3, 4, 5), [2, 3], [2, 3], np.array([6, 6, 8])], eos=EOS)
    assert _arrays(a) == _arrays(b)


def test_fan_out_limit_is_eight_below_the_root():
    t = HW.build_tree(H.SET_FAN, eos=EOS)                        # exactly 8 children: accepted
    assert t.child_off[2] - t.child_off[1] == 8 == HW.MAX_CHILDREN == H.C
    with pytest.raises(ValueError, match="continuations"):
        HW.build_tree([[1, t] for t in range(2, 11)], eos=EOS)   # 9 children of "1"
    many = HW.build_tree([[t] for t in range(1, 40)], eos=99)    # the root may have any number
    assert many.child_off[1] == 39


def test_validation_errors():
    for bad in ([], [[]], [[1, 2], []], [[1, 0, 2]], [[1, EOS]], [[-1]]):
        with pytest.raises(ValueError):
            HW.build_tree(bad, eos=EOS)
    chains = lambda n: [[t] * 10 for t in range(1, n + 1)]       # n chains of 10 nodes + the root
    assert HW.build_tree(chains(6553), eos=10 ** 6).nodes == 65531 <= HW.MAX_NODES == 65535
    with pytest.raises(ValueError, match="65535"):
        HW.build_tree(chains(6554), eos=10 ** 6)                 # 65541 nodes


def test_encode_uses_the_callers_tokenizer():
    table = {"ab": [4, 5], "c": np.array([6])}
    assert HW.encode(["ab", "c"], table.__getitem__) == [[4, 5], [6]]


# ------------------------------------------------------------------------------ scorer walk
WALKS = [
    # phrase set, tokens, k per token, node after
    ("A", [4, 5, 6], [1, 1, 1], 0),                  # a complete phrase (a terminal leaf: back to the root)
    ("A", [4, 5, 9], [1, 1, -2], 0),                 # abandoned after 2 of 3: net 0
    ("A", [4, 5, 4], [1, 1, -1], 2),                 # the mismatching token restarts a phrase: -2 + 1
    ("A", [4, 3], [1, 0], 0),                        # ... and may complete one at once: -1 + 1
    ("A", [4, 5, EOS], [1, 1, -2], 0),               # eos in the middle of a phrase
    ("A", [9, 3, 3, EOS], [0, 1, 1, 0], 0),          # a one-token phrase, twice
    ("B", [2, 3, 4, 9], [1, 1, 1, -1], 0),           # "2 3" was earned: only "4" is taken back
    ("B", [2, 3, 4, 5], [1, 1, 1, 1], 0),
    ("B", [2, 3, EOS], [1, 1, 0], 0),
    ("B", [6, 6, 6, 8], [1, 1, -1, -1], 0),          # "6 6" + 6: -2, restart at "6": +1; then 8 mismatches: -1
    ("B", [6, 6, 8], [1, 1, 1], 0),
    ("B", [0, 6, 0], [0, 1, -1], 0),                 # blank never matches
]


@pytest.mark.parametrize("name,tokens,ks,node", WALKS)
def test_scorer_walk(name, tokens, ks, node):
    """hand-written sequences through the host walk and through the reference tree"""
    assert HW.build_tree(H.SETS[name], eos=EOS).walk(tokens) == (ks, node)
    assert H.Trie(H.SETS[name], EOS).walk(tokens) == (ks, node)


def test_abandoned_phrases_net_zero():
    """whatever is walked, the bonus tokens of a hypothesis that ends (eos) are exactly those of
    the phrases it completed"""
    g = np.random.default_rng(5)
    t = HW.build_tree(H.SETS["AB"], eos=EOS)
    for _ in range(200):
        seq = g.integers(1, EOS, size=12).tolist() + [EOS]
        ks, node = t.walk(seq)
        done, n, run = 0, 0, 0          # completed tokens by direct bookkeeping
        for v in seq:
            m = t.child(n, v)
            if m < 0:
                run = 0
                m = -1 if v == EOS else t.child(0, v)
            if m >= 0:
                run += 1
                if t.terminal[m]:
                    done, run = done + run, 0
                n = m if t.child_off[m] != t.child_off[m + 1] else 0
            else:
                n = 0
        assert sum(ks) == done and node == 0


# ------------------------------------------------------------------------------ set / clear / refuse
def test_set_and_clear_on_the_search():
    bs = get_beam_search_decoder(STUB, TOKENS, ctc_weight=0.3, beam_size=3)
    assert bs.hotwords is None
    bs.set_hotwords(H.SET_A, 2.5)
    assert bs.hotwords.nodes == 6 and bs.hotword_bonus == 2.5
    for clear in (None, []):
        bs.set_hotwords(H.SET_A, 2.5)
        bs.set_hotwords(clear)
        assert bs.hotwords is None and bs.hotword_bonus is None
    for bonus in (None, 0.0, -1.0, float("inf")):                # no default, and a positive number
        with pytest.raises(ValueError):
            bs.set_hotwords(H.SET_A, bonus)
    with pytest.raises(ValueError):
        bs.set_hotwords([[V]], 1.0)                              # outside the vocabulary
    assert bs.hotwords is None
    bs2 = get_beam_search_decoder(STUB, TOKENS, 0.3, 3, H.SET_B, 0.75)
    assert bs2.hotwords.nodes == 8 and bs2.hotword_bonus == 0.75
    with pytest.raises(ValueError):
        get_beam_search_decoder(STUB, TOKENS, 0.3, 3, H.SET_B)


def test_refused_modes_only_with_a_phrase_list():
    for w in (0.0, 1.0):
        bs = get_beam_search_decoder(STUB, TOKENS, ctc_weight=w, beam_size=3)      # fine without a list
        bs.set_hotwords(None)
        bs.set_hotwords([])
        with pytest.raises(NotImplementedError):
            bs.set_hotwords(H.SET_A, 1.0)
        with pytest.raises(NotImplementedError):
            get_beam_search_decoder(STUB, TOKENS, ctc_weight=w, beam_size=3, hotwords=H.SET_A, hotword_bonus=1.0)
    bs = get_beam_search_decoder(STUB, TOKENS, ctc_weight=0.3, beam_size=3, hotwords=H.SET_A, hotword_bonus=1.0)
    with pytest.raises(NotImplementedError):
        bs.stream()
    with pytest.raises(NotImplementedError):
        bs.decode_stream([])
    two = get_rescoring_decoder(STUB, TOKENS, hotwords=None)
    two.set_hotwords(None)
    two.set_hotwords([])
    with pytest.raises(NotImplementedError):
        two.set_hotwords(H.SET_A, 1.0)
    with pytest.raises(NotImplementedError):
        get_rescoring_decoder(STUB, TOKENS, hotwords=H.SET_A, hotword_bonus=1.0)


# ------------------------------------------------------------------------------ the GPU cases
def test_search_cases_are_well_separated_and_cover_the_rules():
    """the conditions on tests/hotword_ref.SEARCH_CASES, from the fp64 reference alone: the values
    the cases must span; every case's smallest top-(beam + 1) gap at least twice the tolerance
    (none skipped); a hypothesis of a final n-best that went through a continuation candidate
    outside the decoder pre-beam; a top hypothesis that differs from the plain search's, carries a
    cancellation and is not the top of the search that never cancels; a completed phrase"""
    assert {(c[1], c[2], c[4]) for c in H.SEARCH_CASES} == {(b, w, beta) for b in (3, 5) for w in (0.1, 0.3)
                                                            for beta in (0.75, 3.0)}
    assert {c[3] for c in H.SEARCH_CASES} == {"A", "B", "AB"} and {c[1] for c in H.CLEARED_CASES} == {3, 5}
    extra = cancel_changes_top = complete = 0
    for case in H.SEARCH_CASES:
        c, refs = H.search_reference(case)
        assert c["Ts"] == [6, 9, 7] and c["V"] == 12
        for hyps, info, plain, nocancel, plain_info in refs:
            assert case not in H.CLEARED_CASES or plain_info["margin"] >= 1.0, (case, plain_info)
            assert hyps and info["margin"] >= 1.0, (case, info)
            assert all(set(h.scores) == {"decoder", "ctc", "hotword"} for h in hyps)
            extra += any("extra" in h.tags for h in hyps)
            complete += any("complete" in h.tags for h in hyps)
            top = hyps[0]
            cancel_changes_top += ("cancel" in top.tags and top.yseq != plain[0].yseq and top.yseq != nocancel[0].yseq)
    assert extra >= 1 and cancel_changes_top >= 1 and complete >= 1, (extra, cancel_changes_top, complete)


def test_reference_without_phrases_is_the_scripted_reference():
    """the biased reference with no phrase list is decode_ref.scripted_search_ref, floats included"""
    c, refs = H.search_reference(H.SEARCH_CASES[0])
    for u, T in enumerate(c["Ts"]):
        want, _ = R.scripted_search_ref(c["table"][u, :T], c["ctc"][u, :T], c["beam"], c["w"])
        got = refs[u][2]
        assert [(h.yseq, h.score, h.scores) for h in got] == [(h.yseq, h.score, h.scores) for h in want]


def test_reference_hotword_score_is_the_walk_of_its_own_tokens():
    """scores["hotword"] of every reference hypothesis = beta * the k of walking its own yseq: every
    token a hypothesis is extended with was one of its row's candidates (an unscored pick would
    sit ~1e9 below); the eos a length limit appends is not walked"""
    for case in H.SEARCH_CASES:
        c, refs = H.search_reference(case)
        trie = H.Trie(c["phrases"], EOS)
        for u, (hyps, info, *_) in enumerate(refs):
            for h in hyps:
                forced = len(h.yseq) - 1 == c["Ts"][u] + 1
                ks, _ = trie.walk(h.yseq[1:-1] if forced else h.yseq[1:])
                assert h.scores["hotword"] == c["beta"] * sum(ks), (case, u, h.yseq)
                total = (1 - c["w"]) * h.scores["decoder"] + c["w"] * h.scores["ctc"] + h.scores["hotword"]
                assert abs(h.score - total) <= 1e-9 * abs(total)

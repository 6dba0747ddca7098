"""The host side of n-gram LM shallow fusion (avsr_amd/ngram_lm.py), without a GPU: ARPA reading
against hand-computed numbers, the compiled arrays against the dict reference of tests/ngram_ref.py
over every short history, argument errors, and what the scripted search cases of ngram_ref cover
(from the fp64 reference's trace alone)."""
import math

import numpy as np
import pytest

from avsr_amd.decode import BatchBeamSearch
from avsr_amd.ngram_lm import NgramLM
from tests import ngram_ref as N

LN10 = math.log(10.0)
TOKS = ["<blank>", "a", "b", "c", "d", "<eos>"]
A, B, C, D, E = 1, 2, 3, 4, 5

ARPA3 = """
\\data\\
ngram 1=6
ngram 2=3
ngram 3=2

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-0.7 a -0.3
-0.8 b -0.2
-1.2 c
-2.0 <unk>

\\2-grams:
-0.4 <s> a -0.1
-0.5 a b -0.25
-0.6 b </s>

\\3-grams:
-0.2 <s> a b
-0.3 a b c

\\end\\
"""


def _close(got, want_log10):
    assert len(got) == len(want_log10)
    for g, w in zip(got, want_log10):
        assert abs(g - w * LN10) <= 1e-6 * abs(w * LN10), (got, want_log10)


# ------------------------------------------------------------------------------ ARPA
def test_arpa_order3_hand_numbers():
    """an order-3 model with <s>, </s>, <unk>, entries with and without a backoff column: the scores
    of three sequences worked out by hand (log10 in the comments), and the compiled shape"""
    lm = NgramLM.from_arpa(ARPA3, TOKS, sos=E, eos=E)
    assert (lm.order, lm.n_vocab, lm.sos, lm.eos) == (3, 6, E, E)
    assert lm.arpa_counts == {1: 6, 2: 3, 3: 2}
    # contexts: (), (<s>), (a), (b), (<s> a), (a b); c has no backoff and no entries below it
    assert sorted(lm.context(n) for n in range(lm.nodes)) == sorted([(), (E,), (A,), (B,), (E, A), (A, B)])
    with pytest.raises(ValueError, match="prefix"):        # "b c d" without "b c"
        NgramLM.from_arpa(ARPA3.replace("-0.3 a b c", "-0.3 a b c\n-0.3 b c d"), TOKS, sos=E, eos=E)
    assert lm.context(lm.start) == (E,) and lm.entries == 5
    assert abs(lm.unk_logp - -2.0 * LN10) < 1e-12
    # a|<s> = -0.4; b|<s> a = -0.2; c|a b = -0.3; then the state is (): </s> = -1.0
    _close(lm.score_tokens([A, B, C]), [-0.4, -0.2, -0.3, -1.0])
    # b|<s>: bo(<s>) -0.5 + b -0.8; d|b: bo(b) -0.2 + <unk> -2.0; </s>|(): -1.0
    _close(lm.score_tokens([B, D]), [-1.3, -2.2, -1.0])
    # a|<s> -0.4; a|<s> a: bo(<s> a) -0.1 + bo(a) -0.3 + a -0.7; </s>|a: bo(a) -0.3 + -1.0
    _close(lm.score_tokens([A, A]), [-0.4, -1.1, -1.3])
    # b </s> is an entry: a b </s> -> bo(a b) -0.25 + -0.6
    _close(lm.score_tokens([A, B])[-1:], [-0.85])
    assert abs(lm.lm_hi - 0.0) < 1e-12                     # every logp and backoff is negative
    assert lm.tok.dtype == lm.child_off.dtype == lm.fail.dtype == lm.next.dtype == lm.uni_next.dtype == np.int32
    assert lm.logp.dtype == lm.backoff.dtype == lm.uni_logp.dtype == np.float32


def test_arpa_from_a_file(tmp_path):
    p = tmp_path / "lm.arpa"
    p.write_text(ARPA3)
    lm = NgramLM.from_arpa(str(p), TOKS, sos=E, eos=E)
    _close(lm.score_tokens([A, B, C]), [-0.4, -0.2, -0.3, -1.0])


def test_arpa_mistyped_path(tmp_path):
    with pytest.raises(FileNotFoundError):
        NgramLM.from_arpa(str(tmp_path / "no_such.arpa"), TOKS, sos=E, eos=E)


def test_arpa_unk_absent_or_given():
    """without <unk>: a vocabulary token without a unigram (d) is an error at load, unless unk_logp
    (natural log) is given, which also overrides the file's <unk>"""
    no_unk = ARPA3.replace("-2.0 <unk>\n", "")
    with pytest.raises(ValueError, match="no unigram"):
        NgramLM.from_arpa(no_unk, TOKS, sos=E, eos=E)
    for text in (no_unk, ARPA3):
        lm = NgramLM.from_arpa(text, TOKS, sos=E, eos=E, unk_logp=-5.0)
        got = lm.score_tokens([B, D])
        assert abs(got[1] - (-0.2 * LN10 - 5.0)) < 1e-6
    # every token has a unigram: neither is needed
    full = no_unk.replace("-1.2 c\n", "-1.2 c\n-1.5 d\n")
    lm = NgramLM.from_arpa(full, TOKS, sos=E, eos=E)
    _close(lm.score_tokens([D])[:1], [-0.5 - 1.5])


def test_arpa_unknown_word_and_bad_lines():
    with pytest.raises(ValueError, match="zzz"):
        NgramLM.from_arpa(ARPA3.replace("-0.5 a b -0.25", "-0.5 a zzz -0.25"), TOKS, sos=E, eos=E)
    with pytest.raises(ValueError, match="ARPA line"):
        NgramLM.from_arpa(ARPA3.replace("-0.5 a b -0.25", "-0.5 a b -0.25 7 8"), TOKS, sos=E, eos=E)
    with pytest.raises(ValueError, match="sections"):
        NgramLM.from_arpa("\\data\\\n\\2-grams:\n-0.5 a b\n\\end\\\n", TOKS, sos=E, eos=E)
    with pytest.raises(ValueError, match="twice"):
        NgramLM.from_arpa(ARPA3.replace("-0.6 b </s>", "-0.6 b </s>\n-0.7 b </s>"), TOKS, sos=E, eos=E)


def test_arpa_sos_with_an_id_of_its_own():
    """sos != eos: <s>'s backoff lands on the id sos, whose own logp is never needed"""
    toks = TOKS + ["<sos>"]
    lm = NgramLM.from_arpa(ARPA3, toks, sos=6, eos=E)
    assert lm.context(lm.start) == (6,)
    _close(lm.score_tokens([B, D]), [-1.3, -2.2, -1.0])


# ------------------------------------------------------------------------------ compiled arrays
def _histories(max_len):
    out = [()]
    for _ in range(max_len):
        out = out + [h + (t,) for h in out if len(h) == len(out[-1]) for t in N.TOKENS]
    return out


@pytest.mark.parametrize("table", ["SEARCH_TABLE", "KERNEL_TABLE"])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_compiled_arrays_equal_dict_reference(table, order):
    """orders 1 - 4, EVERY history of up to 4 of the 10 tokens (after sos): walking the compiled
    arrays from the <s> state reaches the state the dict reference names, and the last token's score
    and successor are the reference's; so is eos after every history of up to 3 tokens. Values of the
    tables lie on a grid of 1/64, so fp32 storage is exact and the comparison is 1e-12."""
    ent = getattr(N, table)
    ref = N.table_lm(ent, order)
    lm = NgramLM.from_table(order, {k: v for k, v in ent.items() if len(k[0]) + 1 <= order}, N.SOS, N.EOS, N.V, N.UNK)
    assert set(ref.contexts) <= {lm.context(n) for n in range(lm.nodes)}     # (the rest: suffixes passed through)
    assert lm.context(lm.start) == ref.state((N.SOS,))
    state = {(): lm.start}
    n = 0
    for h in _histories(4):
        if not h:
            continue
        s, nx = lm.step(state[h[:-1]], h[-1])
        rs, rnx, _ = ref.score(ref.state((N.SOS,) + h[:-1]), h[-1])
        assert abs(s - rs) <= 1e-12 and lm.context(nx) == rnx, (h, s, rs, lm.context(nx), rnx)
        assert lm.state_of((N.SOS,) + h) == nx
        state[h] = nx
        if len(h) <= 3:
            s, nx = lm.step(state[h], N.EOS)
            rs, rnx, _ = ref.score(rnx, N.EOS)
            assert abs(s - rs) <= 1e-12 and lm.context(nx) == rnx, (h, "eos")
        n += 1
    assert n == 10 + 100 + 1000 + 10000
    assert lm.score_tokens([1, 2, 3, 4]) == pytest.approx(ref.score_tokens([1, 2, 3, 4]), abs=1e-12)
    top = max(p for p, _ in ref.entries.values())
    assert lm.lm_hi >= max(0.0, top) and lm.lm_hi >= 0.0


def test_kernel_table_has_the_spans_the_kernel_test_needs():
    lm = NgramLM.from_table(4, N.KERNEL_TABLE, N.SOS, N.EOS, N.V, N.UNK)
    span = {lm.context(n): int(lm.child_off[n + 1] - lm.child_off[n]) for n in range(lm.nodes)}
    assert span[(1,)] == 9 and span[(2,)] == 1 and span[(3,)] == 0 and span[()] == 0
    assert (1, 2, 3) in span and lm.nodes <= 70
    assert float(lm.uni_logp[10]) == N.UNK                 # token 10 has no unigram


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    ok = {((), 1): (-1.0, 0.0)}
    for order in (0, 7):
        with pytest.raises(ValueError, match="order"):
            NgramLM.from_table(order, ok, N.SOS, N.EOS, N.V, N.UNK)
    with pytest.raises(ValueError, match="longer"):
        NgramLM.from_table(1, {((1,), 2): (-1.0, 0.0)}, N.SOS, N.EOS, N.V, N.UNK)
    with pytest.raises(ValueError, match="finite"):
        NgramLM.from_table(1, {((), 1): (float("nan"), 0.0)}, N.SOS, N.EOS, N.V, N.UNK)
    with pytest.raises(ValueError, match="finite"):
        NgramLM.from_table(1, ok, N.SOS, N.EOS, N.V, float("inf"))
    with pytest.raises(ValueError, match="unk_logp"):
        NgramLM.from_table(1, ok, N.SOS, N.EOS, N.V, None)
    with pytest.raises(ValueError, match="outside"):
        NgramLM.from_table(2, {((), 1): (-1.0, 0.0), ((1,), N.V): (-1.0, 0.0)}, N.SOS, N.EOS, N.V, N.UNK)
    with pytest.raises(ValueError, match="outside"):
        NgramLM.from_table(1, ok, N.V, N.EOS, N.V, N.UNK)
    lm = NgramLM.from_table(1, ok, N.SOS, N.EOS, N.V, N.UNK)
    assert lm.nodes == 1 and lm.start == 0 and lm.entries == 0
    with pytest.raises(ValueError, match="outside"):
        lm.score_tokens([N.V])


def _search(w=0.3, V=N.V):
    return BatchBeamSearch(None, beam_size=3, vocab_size=V, weights={"decoder": 1.0 - w, "ctc": w}, sos=V - 1, eos=V - 1,
                           pre_beam_score_key=None if w == 1.0 else "decoder")


def test_set_lm_arguments():
    lm = NgramLM.from_table(2, {k: v for k, v in N.KERNEL_TABLE.items() if len(k[0]) < 2}, N.SOS, N.EOS, N.V, N.UNK)
    bs = _search()
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            bs.set_lm(lm, bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            bs.set_lm(lm, 0.5, bad)
    with pytest.raises(ValueError, match="needs an lm"):
        bs.set_lm(None, 0.5)
    with pytest.raises(ValueError, match="vocabulary"):
        _search(V=N.V + 1).set_lm(lm, 0.5)
    bs.set_lm(lm, 0.5, -0.25)
    assert bs.lm is lm and bs.weights["lm"] == 0.5 and bs.weights["length_bonus"] == -0.25
    assert bs.weights["decoder"] == 0.7 and bs.weights["ctc"] == 0.3
    bs.set_lm(None, 0.0, 1.0)                              # the length bonus alone
    assert bs.lm is None and bs.weights["lm"] == 0.0 and bs.weights["length_bonus"] == 1.0
    bs.set_lm(lm, 0.0)                                     # a scorer of weight 0 is dropped
    assert bs.lm is None
    bs.set_lm(None, 0.0)
    assert bs.lm is None and bs.w_lm == 0.0 and bs.w_len == 0.0
    for w in (0.0, 1.0):
        one = _search(w)
        one.set_lm(None, 0.0)
        with pytest.raises(NotImplementedError, match="two-pass"):
            one.set_lm(lm, 0.5)
        with pytest.raises(NotImplementedError):
            one.set_lm(None, 0.0, 0.5)


# ------------------------------------------------------------------------------ the search cases
def _trace(h):
    orders = {t[1] for t in h.tags if isinstance(t, tuple) and t[0] == "order"}
    left = max([t[1] for t in h.tags if isinstance(t, tuple) and t[0] == "left"] + [0])
    return orders, left


def test_search_cases_cover_what_they_claim():
    """from the fp64 reference's trace alone. Every case (none is skipped): every top-(beam + 1) gap
    of its three searches, and of the three without LM, is at least twice the tolerance; no selected
    token lies outside its row's candidates (where the device's LM term is 0 by definition). Then
    what each row is there for (ngram_ref.CASE_PURPOSE), and across the cases: the winning paths use
    entries of every order of the table, one backs off two levels or more, one hits unk_logp; one
    utterance ends by end detection and one by the length limit."""
    assert len(N.SEARCH_CASES) == len(N.CASE_PURPOSE) == 6
    assert {c[1] for c in N.SEARCH_CASES} == {1, 3, 5}
    orders_won, left_won, ended_by = set(), 0, set()
    per_case = []
    for case in N.SEARCH_CASES:
        c, refs = N.search_reference(case)
        changed, shorter, extra, unk2, left2 = False, False, False, False, False
        for hyps, info, plain, plain_info in refs:
            assert info["margin"] >= 1.0 and plain_info["margin"] >= 1.0, (case, info["margin"], plain_info["margin"])
            assert hyps and plain
            assert not any("unscored" in h.tags for h in hyps + plain), case
            best = hyps[0]
            orders, left = _trace(best)
            if c["lm"] is not None:
                orders_won |= orders
                left_won = max(left_won, left)
                want_keys = {"decoder", "ctc", "lm"} | ({"length_bonus"} if c["w_len"] else set())
                assert set(best.scores) == want_keys | ({"hotword"} if c["phrases"] else set())
            changed |= best.yseq != plain[0].yseq
            shorter |= len(best.yseq) < len(plain[0].yseq)
            extra |= "extra" in best.tags
            unk2 |= 0 in orders and left >= 2
            left2 |= left >= 2
            ended_by.add(info["ended_by"])
        per_case.append(dict(changed=changed, shorter=shorter, extra=extra, unk2=unk2, left2=left2,
                             by={i["ended_by"] for _, i, _, _ in refs}))
    a, b, c5, d, e, f = per_case
    assert a["changed"] and a["unk2"]
    assert b["changed"] and c5["changed"] and c5["left2"] and f["changed"]
    assert d["changed"] and d["shorter"]                       # the length bonus alone changes the best's length
    assert e["by"] == {"end_detect"}
    assert f["extra"]
    assert orders_won >= {0, 1, 2, 3, 4} and left_won >= 2
    assert "end_detect" in ended_by and "limit" in ended_by
    # the LM cases whose tables are not built around an immediate eos: the LM changes the best hypothesis
    assert all(p["changed"] for p, case in zip(per_case, N.SEARCH_CASES) if case[5] is not None and case[3] == "random")



# ------------------------------------------------------------------------------ the parity fixture
def test_reference_fixture_holds_what_it_is_for():
    """tests/golden/avsr_lm.npz, re-asserted from the file: per (setting, clip) the best hypothesis
    differs from the plain golden's yseq_b3_*; neighbouring n-best totals are at least 1e-3 relative
    apart (ten times the comparison tolerance of the GPU test, so rounding does not rank); the best
    path uses entries of order >= 2; the stored scores are the documented sum of their parts, the
    LM score the dict reference's walk and the length bonus the number of scored tokens (the eos a
    length limit appends is not scored)."""
    from tests.oracle_util import load_golden
    fx, g = N.load_lm_fixture(), load_golden()
    V = 5049
    eos = V - 1
    ref = N.RefLM(fx["order"], fx["entries"], fx["unk"], sos=eos, eos=eos)
    lm = NgramLM.from_table(fx["order"], fx["entries"], eos, eos, V, fx["unk"])
    assert len(fx["settings"]) == 2 and fx["settings"][0][1] == 0.0 and fx["settings"][1][1] != 0.0
    unscored = 0
    for (s, c), run in fx["runs"].items():
        w_lm, w_len = fx["settings"][s]
        hyps = run["hyps"]
        T = g[f"dec_enc_{c}"].shape[0]
        assert hyps[0]["yseq"] != g[f"yseq_b3_{c}"].tolist()
        tot = np.array([h["score"] for h in hyps])
        assert len(hyps) >= 2 and np.all(np.diff(tot) < 0)
        assert (np.abs(np.diff(tot)) / np.maximum(np.abs(tot[:-1]), np.abs(tot[1:]))).min() >= 1e-3
        for i, h in enumerate(hyps):
            y = h["yseq"]
            assert y[0] == eos and y[-1] == eos and set(h["scores"]) == {"decoder", "ctc", "lm"} | ({"length_bonus"} if w_len else set())
            forced = len(y) == T + 2                               # sos + T tokens + the appended eos
            scored = y[1:-1] if forced else y[1:]
            unscored += forced
            ctx, total, orders = ref.state((eos,)), 0.0, set()
            for v in scored:
                sc, ctx, (o, _) = ref.score(ctx, v)
                total += sc
                orders.add(o)
            assert abs(h["scores"]["lm"] - total) <= 1e-5 * abs(total)
            assert sum(lm.score_tokens(scored[:-1] if not forced else scored)[:len(scored)]) == pytest.approx(total, rel=1e-6)
            if w_len:
                assert h["scores"]["length_bonus"] == len(scored)
            parts = 0.9 * h["scores"]["decoder"] + 0.1 * h["scores"]["ctc"] + w_lm * h["scores"]["lm"] + w_len * len(scored)
            assert abs(h["score"] - parts) <= 1e-5 * abs(parts)
            if i == 0:
                assert max(orders) >= 2
    assert unscored > 0                                            # the unscored-eos rule is in the fixture

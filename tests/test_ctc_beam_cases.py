"""The cases of the avsr_ctc_beam kernel tests, judged from the fp64 restatement alone
(tests/ctc_beam_ref.py): every configuration keeps its skip share under the cap, and between
them the cases meet every event the kernel has to get right. No library call."""
import numpy as np
import pytest

from tests import ctc_beam_ref as R

ALL_CONFIGS = [(kind, N, C) for kind, cfgs in R.CONFIGS.items() for N, C in cfgs]


@pytest.mark.parametrize("kind,N,C", ALL_CONFIGS)
def test_skip_share_under_cap(kind, N, C):
    cases = R.config_cases(kind, N, C)
    skipped = sum(c["ref"]["margin"] < 1 for c in cases)
    assert len(cases) == R.SEEDS_PER_CONFIG
    assert skipped <= R.MAX_SKIP_SHARE * len(cases), (kind, N, C, skipped)


def test_extra_cases_do_not_skip():
    assert all(c["ref"]["margin"] >= 1 for c in R.extra_cases())


def _events():
    seen = {}
    cases = [c for kind, N, C in ALL_CONFIGS for c in R.config_cases(kind, N, C)] + R.extra_cases()
    for c in cases:
        if c["ref"]["margin"] >= 1:
            for e in c["ref"]["events"]:
                seen[e] = seen.get(e, 0) + 1
    return seen


@pytest.mark.parametrize("event", R.EVENTS)
def test_event_is_met(event):
    """repeat-token split, merge of an extension into a prefix already in the beam, merge with a
    re-created prefix, the empty prefix surviving to the end, candidate lists holding blank / eos"""
    assert _events().get(event, 0) > 0, event


def test_n_out_below_beam_at_one_frame():
    """N = 16 with one frame: at most 1 + C entries exist"""
    logp = R.make_case(R.FIRST_SEED, "peaked", T=1)
    ref = R.search(logp, R.topk_ids(logp, 4), 16)
    assert 1 <= len(ref["hyps"]) <= 5 < 16
    assert ref["hyps"][0][1] >= ref["hyps"][-1][1]


def test_restatement_on_a_hand_case():
    """two frames, tokens {blank, 1}: P(()) = p0(b) p1(b); P((1,)) = everything else that
    collapses to one token; (1, 1) needs a blank between and has no path"""
    p = np.full((2, R.V), 1e-30)
    p[0, 0], p[0, 1] = 0.6, 0.4
    p[1, 0], p[1, 1] = 0.3, 0.7
    logp = np.log(p).astype(np.float32)
    cand = np.array([[1, 0], [1, 0]], dtype=np.int32)
    ref = R.search(logp, cand, 4)
    got = {h: s for h, s in ref["hyps"]}
    q = np.exp(logp.astype(np.float64))
    assert got[()] == pytest.approx(np.log(q[0, 0] * q[1, 0]), abs=1e-12)
    assert got[(1,)] == pytest.approx(np.log(q[0, 1] * q[1, 0] + q[0, 0] * q[1, 1] + q[0, 1] * q[1, 1]), abs=1e-12)
    assert got[(1, 1)] == float("-inf")       # entered through pb = -inf: no path yet

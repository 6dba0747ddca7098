"""avsr_ctc_beam (CTC prefix beam search, one launch for a batch of utterances) against the fp64
restatement tests/ctc_beam_ref.py. Which cases are compared is decided by the restatement alone
(its margin rule); tests/test_ctc_beam_cases.py checks, without a GPU, that few are skipped and
that the cases meet every merge / split event."""
import numpy as np
import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import ops
from tests import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

ALL_CONFIGS = [(kind, N, C) for kind, cfgs in R.CONFIGS.items() for N, C in cfgs]


def run(dev, cases, N, C, Lcap=None, V=R.V, blank=R.BLANK, eos=R.EOS, Tm=None):
    """one launch over `cases` (dicts with logp (T, V) and cand (T, C); T = 0 allowed). Padding
    frames hold log-prob 0 everywhere and a valid token as every candidate: reading one of them
    would change every score. -> host (n_out, tokens, len, score)"""
    U = len(cases)
    Ts = [c["logp"].shape[0] for c in cases]
    Tm = max(Ts + [1]) if Tm is None else Tm
    logp = np.zeros((U, Tm, V), dtype=np.float32)
    cand = np.full((U, Tm, C), 3, dtype=np.int32)
    for u, c in enumerate(cases):
        logp[u, :Ts[u]] = c["logp"]
        cand[u, :Ts[u]] = c["cand"]
    out = ops.ctc_beam(torch.from_numpy(logp).to(dev), torch.tensor(Ts, dtype=torch.int32).to(dev),
                       torch.from_numpy(cand).to(dev), N, blank=blank, eos=eos, Lcap=Lcap)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def check(case, ref, out, u, N):
    """utterance u of a launch against its reference: sequences, lengths, order, n_out, scores
    within tol, fill values"""
    n_out, tokens, length, score = out
    hyps, T = ref["hyps"], case["logp"].shape[0]
    assert n_out[u] == len(hyps)
    for r, (toks, s) in enumerate(hyps):
        assert length[u, r] == len(toks), (r, toks)
        assert tuple(tokens[u, r, :len(toks)].tolist()) == toks, (r, toks)
        assert (tokens[u, r, len(toks):] == -1).all()
        got = float(score[u, r])
        print(f"u{u} r{r} len {len(toks)} score {got:.6f} ref {s:.6f} tol {R.tol(s, T):.2e}")
        if s == R.NEG_INF:
            assert got == R.NEG_INF
        else:
            assert abs(got - s) <= R.tol(s, T), (r, got, s)
    assert (tokens[u, len(hyps):] == -1).all() and (length[u, len(hyps):] == 0).all()
    assert np.isneginf(score[u, len(hyps):]).all()


@pytest.mark.parametrize("kind,N,C", ALL_CONFIGS)
def test_against_restatement(dev, kind, N, C):
    """U = 4 utterances of different lengths per launch"""
    cases = R.config_cases(kind, N, C)
    compared = 0
    for g in range(0, len(cases), 4):
        group = cases[g:g + 4]
        out = run(dev, group, N, C)
        for u, c in enumerate(group):
            if c["ref"]["margin"] >= 1:
                check(c, c["ref"], out, u, N)
                compared += 1
    assert compared >= (1 - R.MAX_SKIP_SHARE) * len(cases)


def test_extra_cases(dev):
    """the re-created-prefix merges and the surviving empty prefix"""
    for c in R.extra_cases():
        assert c["ref"]["margin"] >= 1
        check(c, c["ref"], run(dev, [c], c["N"], c["C"]), 0, c["N"])


def test_one_frame(dev):
    logp = R.make_case(R.FIRST_SEED, "peaked", T=1)
    c = dict(logp=logp, cand=R.topk_ids(logp, 4))
    ref = R.search(logp, c["cand"], 16)
    assert ref["margin"] >= 1 and len(ref["hyps"]) < 16
    check(c, ref, run(dev, [c], 16, 4), 0, 16)


def test_empty_utterance_in_a_batch(dev):
    cases = R.config_cases("peaked", 4, 8)[:3]
    assert all(c["ref"]["margin"] >= 1 for c in cases)
    empty = dict(logp=np.zeros((0, R.V), np.float32), cand=np.zeros((0, 8), np.int32))
    group = [cases[0], empty, cases[1], cases[2]]
    out = run(dev, group, 4, 8)
    assert out[0][1] == 0 and (out[1][1] == -1).all() and (out[2][1] == 0).all() and np.isneginf(out[3][1]).all()
    for u in (0, 2, 3):
        check(group[u], group[u]["ref"], out, u, 4)


def test_length_cap_binds(dev):
    N, C, Lcap = 4, 8, 3
    for seed in range(R.FIRST_SEED, R.FIRST_SEED + 40):      # the first case the cap changes, by the restatement
        c = R.case("peaked", N, C, seed)
        ref = R.search(c["logp"], c["cand"], N, Lcap=Lcap)
        if ref["margin"] >= 1 and c["ref"]["margin"] >= 1 and [h for h, _ in ref["hyps"]] != [h for h, _ in c["ref"]["hyps"]]:
            break
    else:
        pytest.fail("no case where the cap binds")
    assert max(len(h) for h, _ in ref["hyps"]) == Lcap < max(len(h) for h, _ in c["ref"]["hyps"])
    out = run(dev, [c], N, C, Lcap=Lcap)
    assert out[1].shape == (1, N, Lcap)
    check(c, ref, out, 0, N)


def test_alone_and_in_a_batch_bit_identical(dev):
    cases = R.config_cases("randn3", 10, 16)[:4]
    batch = run(dev, cases, 10, 16)
    Tm = max(c["T"] for c in cases)
    for u, c in enumerate(cases):
        alone = run(dev, [c], 10, 16, Lcap=min(Tm, 511))
        assert alone[0][0] == batch[0][u]
        assert (alone[1][0] == batch[1][u]).all() and (alone[2][0] == batch[2][u]).all()
        assert (alone[3][0].view(np.int32) == batch[3][u].view(np.int32)).all()


LONG_T, LONG_V, LONG_N, LONG_C = 400, 5049, 4, 16


def test_long_utterance_real_vocabulary(dev):
    """T = 400 frames over V = 5049 with C = 16 candidates from the engine's own top-k: the
    workspace at its real size, token ids beyond a byte, and the restatement fed the very
    log-prob bits the kernel reads. Peaked logits (3 * randn with +32 on one token per frame,
    blank half the time) and N = 4 keep the restatement's margin above 1 over 400 cuts (about 8
    with a host log-softmax; at N = 8 the same inputs come to 1.3)."""
    rng = np.random.default_rng(R.FIRST_SEED)
    x = (3.0 * rng.standard_normal((LONG_T, LONG_V))).astype(np.float32)
    for t in range(LONG_T):
        x[t, 0 if rng.random() < 0.5 else int(rng.integers(1, LONG_V - 1))] += 32.0
    logits = torch.zeros(LONG_T, (LONG_V + 7) // 8 * 8, device=dev)
    logits[:, :LONG_V] = torch.from_numpy(x).to(dev)
    logp = torch.empty(1, LONG_T, LONG_V, device=dev, dtype=torch.float32)
    cand = torch.empty(1, LONG_T, LONG_C, device=dev, dtype=torch.int32)
    ops.log_softmax_topk(logits, LONG_V, logp.view(LONG_T, LONG_V), LONG_C, cand.view(LONG_T, LONG_C))
    out = ops.ctc_beam(logp, torch.tensor([LONG_T], dtype=torch.int32).to(dev), cand, LONG_N, blank=0, eos=LONG_V - 1)
    torch.cuda.synchronize()
    out = tuple(o.cpu().numpy() for o in out)
    c = dict(logp=logp[0].cpu().numpy(), cand=cand[0].cpu().numpy())
    assert (c["cand"] == R.topk_ids(c["logp"], LONG_C)).all()
    ref = R.search(c["logp"], c["cand"], LONG_N, blank=0, eos=LONG_V - 1, Lcap=min(LONG_T, 511))
    assert ref["margin"] >= 1, ref["margin"]
    assert out[1].shape == (1, LONG_N, LONG_T)
    check(c, ref, out, 0, LONG_N)


def test_limits(dev):
    c = R.case("peaked", 4, 8, R.FIRST_SEED)
    with pytest.raises(L.AvsrLibError, match="1001"):          # AVSR_E_SHAPE
        run(dev, [c], 17, 8)
    wide = dict(logp=c["logp"], cand=R.topk_ids(c["logp"], 17))
    with pytest.raises(L.AvsrLibError, match="1001"):
        run(dev, [wide], 4, 17)
    with pytest.raises(L.AvsrLibError, match="1001"):
        run(dev, [c], 4, 8, Lcap=512)

"""avsr_ngram_step and avsr_ngram_score_seqs (csrc/ngram.hip) against the dict reference of
tests/ngram_ref.py: floats at 1e-6 relative, successor states exact. The table is
ngram_ref.KERNEL_TABLE cut to orders 1 - 4 (spans of 0, 1 and 9 entries, a full-depth backoff
chain, a token without a unigram; tests/test_ngram_host.py checks that it has them)."""
import numpy as np
import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import ops
from avsr_amd.ngram_lm import NgramLM
from tests import ngram_ref as N

pytestmark = pytest.mark.gpu


def _lms(order):
    ent = {k: v for k, v in N.KERNEL_TABLE.items() if len(k[0]) + 1 <= order}
    return NgramLM.from_table(order, ent, N.SOS, N.EOS, N.V, N.UNK), N.table_lm(N.KERNEL_TABLE, order)


# the looked-up token first (1), last (9) and absent (10, which has no unigram either) in the
# 9-entry span of node (1,); blank (padding) and eos as ids columns
BASE_IDS = [1, 9, 10, 5, 0, 11, 3, 2, 4, 6, 7, 8]


def _ids(R, P):
    return np.array([[BASE_IDS[(r + c + (c // 12) * r) % 12] for c in range(P)] for r in range(R)], np.int32)


@pytest.mark.parametrize("R,P", [(1, 1), (1, 7), (70, 1), (70, 7), (70, 63)], ids=lambda v: str(v))
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_ngram_step_matches_reference(dev, order, R, P):
    """rows placed in every context of the table in turn (R = 70 > the number of nodes), the last two
    rows at out-of-range states (read as <s>); every column against the reference"""
    lm, ref = _lms(order)
    real = [n for n in range(lm.nodes) if lm.context(n) in ref.contexts]
    assert len(real) == len(ref.contexts) <= 70
    states = [real[(r + 3) % len(real)] for r in range(R)]
    if R > 1:
        states[-1], states[-2] = -1, lm.nodes + 5
    ctx = [lm.context(s) if 0 <= s < lm.nodes else ref.state((N.SOS,)) for s in states]
    ids = _ids(R, P)
    if R == 1 and P == 7:
        states, ctx = [lm.state_of((N.SOS, 1, 2, 3))], [ref.state((N.SOS, 1, 2, 3))]     # the deepest context
    arr = ops.ngram_arrays(lm, dev)
    out = torch.full((R, P + 1), 7.0, device=dev)
    nxt = torch.full((R, P + 1), -7, device=dev, dtype=torch.int32)
    ops.ngram_step(arr, torch.tensor(states, dtype=torch.int32).to(dev), torch.from_numpy(ids).to(dev), out, nxt,
                   blank=N.BLANK, eos=N.EOS)
    out, nxt = out.cpu().numpy(), nxt.cpu().numpy()
    want, want_next = N.ngram_step_ref(ref, ctx, ids)
    assert np.all(np.abs(out - want) <= 1e-6 * np.abs(want)), np.abs(out - want).max()
    for r in range(R):
        for c in range(P + 1):
            assert lm.context(int(nxt[r, c])) == want_next[r][c], (r, c, states[r], ids[r].tolist())
            if c < P and ids[r, c] == N.BLANK:
                assert out[r, c] == 0.0 and (nxt[r, c] == states[r] or not 0 <= states[r] < lm.nodes)
    if order == 4 and R == 1 and P == 7:
        # 10 after (1, 2, 3): three contexts left, then unk_logp, the backoffs added in that order
        bo = [ref.backoff((1, 2, 3)), ref.backoff((2, 3)), ref.backoff((3,))]
        assert bo[0] != 0.0 and bo[2] != 0.0
        assert out[0, 2] == np.float32(np.float32(np.float32(bo[0]) + np.float32(bo[1])) + np.float32(bo[2])) + \
            np.float32(N.UNK)


def test_ngram_step_error_returns(dev):
    lm, _ = _lms(3)
    arr = ops.ngram_arrays(lm, dev)
    i32 = dict(device=dev, dtype=torch.int32)

    def call(arr=arr, P=3, **nulls):
        kw = dict(state=torch.zeros(2, **i32), ids=torch.ones(2, P, **i32), out=torch.zeros(2, P + 1, device=dev),
                  out_next=torch.zeros(2, P + 1, **i32))
        kw.update(nulls)
        p = L.fill(L.NgramParams, lm=ops._ngram_struct(arr), R=2, P=P, blank=0, eos=N.EOS, **kw)
        return L.load().avsr_ngram_step(p, None)

    assert call() == 0
    assert call(P=63) == 0 and call(P=64) == 1001                           # AVSR_E_SHAPE: W > 64
    for k, v in (("order", 0), ("order", 7), ("nodes", 0)):
        assert call(arr={**arr, k: v}) == 1001, (k, v)
    for k in ("state", "ids", "out", "out_next"):
        assert call(**{k: None}) == 1004, k                                # AVSR_E_ARG: a NULL array
    assert call(arr={**arr, "tok": torch.zeros(0, **i32)}) == 1004          # tok NULL, logp / next not: all or none
    assert L.load().avsr_ngram_step(None, None) == 1004
    assert L.load().avsr_ngram_score_seqs(None, None) == 1004
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("order", [1, 4])
def test_score_seqs_equals_the_step_kernel_walk(dev, order, n):
    """hypotheses of 0, 1, .. cap tokens, -1 padded: every value == the step kernel walked token by
    token from the <s> state (the two kernels share the lookup), 0 beyond the closing eos; and both
    are the reference's numbers"""
    lm, ref = _lms(order)
    arr = ops.ngram_arrays(lm, dev)
    cap = 6
    lens = [0, 1, cap][:n] if n < 4 else [(b * 5) % (cap + 1) for b in range(n)]
    assert {0, 1, cap} <= set(lens) or n == 1
    seqs = [[[1, 2, 3, 4, 10, 1, 9, 5][(b + j) % 8] for j in range(ln)] for b, ln in enumerate(lens)]
    toks = torch.full((n, cap), -1, dtype=torch.int32)
    for b, y in enumerate(seqs):
        toks[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
    got = ops.ngram_score_seqs(arr, toks.to(dev), eos=N.EOS).cpu().numpy()
    assert got.shape == (n, cap + 1)
    state = torch.full((n,), lm.start, dtype=torch.int32, device=dev)
    walked = np.zeros((n, cap + 1), np.float32)
    for j in range(cap + 1):
        col = torch.tensor([[y[j] if j < len(y) else N.EOS] for y in seqs], dtype=torch.int32).to(dev)
        out = torch.empty(n, 2, device=dev)
        nxt = torch.empty(n, 2, device=dev, dtype=torch.int32)
        ops.ngram_step(arr, state, col, out, nxt, blank=N.BLANK, eos=N.EOS)
        o = out.cpu().numpy()
        for b, y in enumerate(seqs):
            if j <= len(y):
                walked[b, j] = o[b, 0]
        state = nxt[:, 0].contiguous()
    assert np.array_equal(got, walked)
    for b, y in enumerate(seqs):
        want = ref.score_tokens(y)
        assert np.all(np.abs(got[b, :len(y) + 1] - want) <= 1e-6 * np.abs(want)) and np.all(got[b, len(y) + 1:] == 0.0)


def test_model_with_unigrams_only_runs(dev):
    """an order-2 model that lists only unigrams has contexts (those with a backoff, and <s>) but no
    entry below the unigram level: the entry arrays are NULL and every lookup backs off"""
    ent = {((), v): (-1.0 - 0.25 * v, -0.5 if v in (2, N.EOS) else 0.0) for v in (1, 2, 3, N.EOS)}
    lm = NgramLM.from_table(2, ent, N.SOS, N.EOS, N.V, N.UNK)
    ref = N.RefLM(2, ent, N.UNK)
    assert lm.nodes == 3 and lm.entries == 0
    arr = ops.ngram_arrays(lm, dev)
    states = [lm.start, lm.state_of((N.SOS, 2)), 0]
    ids = np.array([[1, 2, 9]] * 3, np.int32)
    out = torch.empty(3, 4, device=dev)
    nxt = torch.empty(3, 4, device=dev, dtype=torch.int32)
    ops.ngram_step(arr, torch.tensor(states, dtype=torch.int32).to(dev), torch.from_numpy(ids).to(dev), out, nxt,
                   blank=N.BLANK, eos=N.EOS)
    want, want_next = N.ngram_step_ref(ref, [lm.context(s) for s in states], ids)
    assert np.all(np.abs(out.cpu().numpy() - want) <= 1e-6 * np.abs(want))
    assert [[lm.context(int(n)) for n in row] for row in nxt.cpu().numpy()] == want_next
    seq = ops.ngram_score_seqs(arr, torch.tensor([[2, 1]], dtype=torch.int32).to(dev), eos=N.EOS).cpu().numpy()[0]
    assert np.all(np.abs(seq - ref.score_tokens([2, 1])) <= 1e-6 * np.abs(ref.score_tokens([2, 1])))

"""avsr_ctc_neighbors on the device against tests/confidence_ref.py: the CTC likelihood of every
one-edit neighbour's explicit label sequence (torch ctc_loss, fp64), which knows nothing of the
kernel's shared alpha / beta. Conventions of tests/test_gpu_align.py: logits are 1e30 in columns
>= V and frames >= in_len[b] (a stray read shows), every output and the workspace start as
garbage (an unwritten element shows).

Tolerance on the finite scores: the project's bound for fp32 log-space CTC against fp64,
max-normalised error < 1e-5 (tests/test_gpu_loss_misc.py::test_ctc), 1e-3 for bf16 logits; the
reference sees the same device-rounded logits, upcast. Measured on an MI355X: at most 4.3e-7 in the
T <= 50 launches (fp32 and bf16 alike) and 1.0e-6 at T = 375, L = 40, V = 5049, so the
bound stands as it is."""
import pytest
import torch

from avsr_amd import _lib as L
from avsr_amd import ops
from tests import confidence_ref as R

pytestmark = pytest.mark.gpu

BIG = 1e30
NEG_INF = float("-inf")
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-3}


def _inputs(cases, T, V, ldx, dtype, seed=0):
    B = len(cases)
    x = torch.randn(B * T, ldx, generator=torch.Generator().manual_seed(seed)) * 3
    x[:, V:] = BIG
    for b, (Tb, _) in enumerate(cases):
        x[b * T + max(Tb, 0):(b + 1) * T] = BIG
    x = x.to(dtype)
    return x, torch.logsumexp(x.float()[:, :V], -1)


def _launch(dev, x, lse, cases, T, V, lds, eos, blank=0, Lmax=None, with_lz=True):
    B = len(cases)
    Lmax = max(1, max(len(y) for _, y in cases)) if Lmax is None else Lmax
    lab = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, (_, y) in enumerate(cases):
        lab[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
    sub = torch.full((B, Lmax, lds), 7777.0, device=dev)
    dele = torch.full((B, Lmax), 7777.0, device=dev)
    base = torch.full((B,), 7777.0, device=dev)
    feas = torch.full((B,), 7777, dtype=torch.int32, device=dev)
    lz = torch.full((B, Lmax), 7777.0, device=dev) if with_lz else None
    ws = torch.full((max(16, ops.ctc_neighbors_ws(B, T, Lmax)),), 255, dtype=torch.uint8, device=dev)
    ops.ctc_neighbors(x.to(dev), B, T, V, lab.to(dev), torch.tensor([len(y) for _, y in cases], dtype=torch.int32).to(dev),
                      torch.tensor([Tb for Tb, _ in cases], dtype=torch.int32).to(dev), lse.to(dev), blank=blank,
                      eos=eos, sub=sub, dele=dele, base=base, feasible=feas, ws=ws, lz=lz)
    return sub.cpu(), dele.cpu(), base.cpu(), feas.cpu(), None if lz is None else lz.cpu()


def _logp64(x, b, T, V):
    return torch.log_softmax(x[b * T:(b + 1) * T, :V].double(), -1)


def _close(got, want, tol, what):
    """-inf exactly where the reference is -inf; the finite scores within tol of the largest |reference|"""
    got, want = got.double(), want.double()
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), (what, "-inf pattern", (got[inf] != want[inf]).nonzero()[:8])
    if (~inf).any():
        assert torch.isfinite(got[~inf]).all(), (what, "finite expected")
        err = ((got[~inf] - want[~inf]).abs().max() / want[~inf].abs().max().clamp_min(1e-30)).item()
        print(f"{what}: max-normalised error {err:.3e}")
        assert err < tol, (what, err, tol)


def _expect_feasible(Tb, y, V, blank=0):
    return Tb > 0 and all(0 <= t < V and t != blank for t in y) and Tb >= len(y) + sum(a == b for a, b in zip(y, y[1:]))


def _check(got, x, cases, T, V, eos, tol, blank=0):
    sub, dele, base, feas, lz = got
    for b, (Tb, y) in enumerate(cases):
        Ly = len(y)
        ok = _expect_feasible(Tb, y, V, blank)
        assert feas[b].item() == int(ok), (b, feas[b])
        assert torch.isinf(sub[b, :, V:]).all() and torch.isinf(sub[b, Ly:]).all() and (sub[b] < 0).all(), b
        assert torch.isinf(sub[b, :, blank]).all() and (eos < 0 or torch.isinf(sub[b, :, eos]).all()), b
        assert (dele[b, Ly:] == NEG_INF).all(), b
        if not ok:
            assert base[b].item() == 0.0 and (sub[b] == NEG_INF).all() and (dele[b] == NEG_INF).all(), b
            assert lz is None or (lz[b] == NEG_INF).all(), b
            continue
        rs, rd, rb = R.neighbors(_logp64(x, b, T, V), y, Tb, blank, eos)
        _close(base[b:b + 1], torch.tensor([rb]), tol, f"utt {b} base")
        if Ly:
            _close(sub[b, :Ly, :V], rs, tol, f"utt {b} sub")
            _close(dele[b, :Ly], rd, tol, f"utt {b} del")
            own = sub[b, torch.arange(Ly), torch.tensor(y)]
            _close(own, base[b].expand(Ly), tol, f"utt {b} sub[l][y_l] = base")
        if lz is not None:
            # Z_l - base from the kernel's OWN scores in fp64: fp32 rounding of a value near 0
            assert (lz[b, Ly:] == NEG_INF).all(), b
            for l in range(Ly):
                z = torch.logsumexp(torch.cat([sub[b, l, :V].double(), dele[b, l].double().view(1)]), 0) - base[b].double()
                assert abs(lz[b, l].item() - z.item()) <= 1e-6 * max(1.0, abs(z.item())), (b, l, lz[b, l], z)


V1, T1, LD1, EOS1 = 11, 9, 16, 10
LAUNCH1 = [(9, (3, 3, 5, 2)),      # a repeat: v = y_{l-1}, v = y_{l+1}, and v = 3 at slot 3 makes a triple
           (5, (3, 3, 5, 2)),      # tight, n = L + repeats: every neighbour that adds a repeat is -inf
           (4, (3, 3, 5, 2)),      # no path
           (6, (4, 9, 4)),         # y_{l-1} = y_{l+1}: the deletion creates a repeat; v = 4 at slot 2
           (9, (7,)), (1, (7,)),   # L = 1; n = 1
           (5, ()),                # no slots
           (0, (2,)),              # in_len = 0
           (9, (3, V1, 2))]        # a label = V


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_small_launch(dev, dtype):
    x, lse = _inputs(LAUNCH1, T1, V1, LD1, dtype)
    got = _launch(dev, x, lse, LAUNCH1, T1, V1, LD1, EOS1)
    _check(got, x, LAUNCH1, T1, V1, EOS1, TOL[dtype])
    sub, dele, base, feas, _ = got
    assert feas.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 0]
    # the tight utterance: a substitute equal to a neighbour adds a repeat the 5 frames cannot separate
    assert sub[1, 2, 3].item() == NEG_INF and sub[1, 2, 2].item() == NEG_INF and sub[1, 3, 5].item() == NEG_INF
    assert torch.isfinite(sub[1, 1, 4]) and torch.isfinite(sub[1, 0, 4])       # ... one that removes it is not
    assert torch.isfinite(sub[0, 2, 3])                                         # the triple, with frames to spare
    assert dele[3, 1].item() > NEG_INF and torch.isfinite(dele[1]).all()
    # base is the loss kernel's likelihood of the same labels
    live = [b for b in range(len(LAUNCH1)) if feas[b]]
    Lmax = sub.shape[1]
    lab = torch.zeros(len(live), Lmax, dtype=torch.int32)
    for i, b in enumerate(live):
        lab[i, :len(LAUNCH1[b][1])] = torch.tensor(LAUNCH1[b][1], dtype=torch.int32)
    rows = torch.cat([torch.arange(b * T1, (b + 1) * T1) for b in live])
    nll = torch.zeros(len(live), device=dev)
    alpha = torch.empty(len(live), T1, 2 * Lmax + 1, device=dev)
    ops.ctc_fwd(ops.ctc_params(x[rows].to(dev), len(live), T1, V1, lab.to(dev),
                               torch.tensor([len(LAUNCH1[b][1]) for b in live], dtype=torch.int32).to(dev),
                               torch.tensor([LAUNCH1[b][0] for b in live], dtype=torch.int32).to(dev), lse[rows].to(dev),
                               alpha, torch.empty_like(alpha), nll))
    _close(base[live], -nll.cpu(), TOL[dtype], "base = -nll of avsr_ctc_fwd")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_independence_bitwise(dev, dtype):
    """each utterance launched alone (B = 1, its own Lmax) gives bit-identical outputs"""
    x, lse = _inputs(LAUNCH1, T1, V1, LD1, dtype)
    sub, dele, base, feas, lz = _launch(dev, x, lse, LAUNCH1, T1, V1, LD1, EOS1)
    for b, case in enumerate(LAUNCH1):
        s1, d1, b1, f1, z1 = _launch(dev, x[b * T1:(b + 1) * T1], lse[b * T1:(b + 1) * T1], [case], T1, V1, LD1, EOS1)
        n = max(1, len(case[1]))
        assert f1[0] == feas[b]
        for one, full in ((s1[0, :n], sub[b, :n]), (d1[0, :n], dele[b, :n]), (b1[0], base[b]), (z1[0, :n], lz[b, :n])):
            assert torch.equal(one.contiguous().view(torch.int32), full.contiguous().view(torch.int32)), b


def test_no_eos_leaves_the_column_scored(dev):
    x, lse = _inputs(LAUNCH1, T1, V1, LD1, torch.float32)
    got = _launch(dev, x, lse, LAUNCH1, T1, V1, LD1, -1, with_lz=False)
    _check(got, x, LAUNCH1, T1, V1, -1, 1e-5)
    assert torch.isfinite(got[0][0, :4, EOS1]).all() and torch.isfinite(got[0][4, 0, EOS1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_production_vocabulary(dev, dtype):
    """V = 5049 / ldx = 5056: the lane tail at V mod 64 != 0, ids at both ends, the tile edges"""
    cases = [(50, (5, 5, 17, 301, 4000, 17)), (41, (77, 5047, 1, 2))]
    V, T, ld = 5049, 50, 5056
    x, lse = _inputs(cases, T, V, ld, dtype, seed=3)
    _check(_launch(dev, x, lse, cases, T, V, ld, V - 1), x, cases, T, V, V - 1, TOL[dtype])


def test_long_recursion(dev):
    """T = 375, L = 40 with one adjacent repeat, V = 5049: every chunk boundary over t (6 chunks of
    64 frames in the substitution kernel, 8 emission chunks in the alpha / beta kernel). Full rows
    for the second label of the repeat and the last slot; for all 40 slots the 64 columns made of
    y's own tokens plus the first ids from 1 up; del for all slots."""
    V, T, ld, Ly = 5049, 375, 5056, 40
    g = torch.Generator().manual_seed(11)
    y = (torch.randperm(V - 2, generator=g)[:Ly] + 1).tolist()
    y[11] = y[10]
    cases = [(T, tuple(y))]
    x, lse = _inputs(cases, T, V, ld, torch.float32, seed=5)
    sub, dele, base, feas, _ = _launch(dev, x, lse, cases, T, V, ld, V - 1, with_lz=False)
    assert feas.tolist() == [1]
    logp = _logp64(x, 0, T, V)
    rs, rd, rb = R.neighbors(logp, y, T, 0, V - 1, slots={11, Ly - 1})
    _close(base, torch.tensor([rb]), 1e-5, "base")
    _close(dele[0], rd, 1e-5, "del")
    _close(sub[0, [11, Ly - 1], :V], rs[[11, Ly - 1]], 1e-5, "sub, full rows of slots 12 and 40")
    cols = sorted(set(y))
    cols += [c for c in range(1, 200) if c not in set(y)][:64 - len(cols)]
    rs, _, _ = R.neighbors(logp, y, T, 0, V - 1, cols=cols)
    _close(sub[0, :, cols], rs[:, cols], 1e-5, "sub, 64 columns of every slot")
    own = sub[0, torch.arange(Ly), torch.tensor(y)]
    _close(own, base.expand(Ly), 1e-5, "sub[l][y_l] = base")


def test_shape_and_alignment_errors(dev):
    """host-side returns, nothing launched: 2 Lmax + 1 > 1024, and a workspace off its alignment"""
    cases = [(9, (3, 5))]
    x, lse = _inputs(cases, T1, V1, LD1, torch.float32)
    with pytest.raises(L.AvsrLibError, match="1001"):            # AVSR_E_SHAPE
        _launch(dev, x, lse, cases, T1, V1, LD1, EOS1, Lmax=512)
    lab = torch.tensor([[3, 5]], dtype=torch.int32, device=dev)
    one = torch.tensor([2], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.ctc_neighbors_ws(1, T1, 2) + 16, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    with pytest.raises(L.AvsrLibError, match="1002"):            # AVSR_E_ALIGN
        ops.ctc_neighbors(x.to(dev), 1, T1, V1, lab, one, torch.tensor([9], dtype=torch.int32, device=dev), lse.to(dev),
                          eos=EOS1, ws=ws[4:])

"""The loss kernels of avsr_amd/csrc/loss.hip at their launch edges: avsr_row_lse, avsr_lsm_fwd,
avsr_lsm_bwd, avsr_ctc_fwd, avsr_ctc_bwd and avsr_loss_finalize against plain fp64 references
(tests/ctc_loss_ref.py for CTC), with NaN in every padded column the kernels must not read and
NaN in every output they must write. References come from the stored (device-rounded) logits."""
import functools

import pytest
import torch

from avsr_amd import ops, _lib as L
from tests import ctc_loss_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")


def _maxerr(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


def _zero(t):
    """every element is exactly 0 (NaN is not); true of an empty tensor"""
    return t.numel() == 0 or t.abs().max().item() == 0


# ------------------------------------------------------------------------------------- CTC
@functools.lru_cache(maxsize=None)
def _ctc_refs(name, regime, dtype):
    """per utterance of a case: the fp64 reference of the stored logits, the fp32 error of the same
    recursion on gamma (e32_gamma) and torch's fp32 ctc_loss error on the gradient, relative to
    the largest reference gradient (e32)"""
    c = R.CTC_CASES[name]
    x = R.case_logits(name, regime, dtype)
    out = []
    for b, (labels, in_len) in enumerate(c["utts"]):
        xb = x[b, :, :c["V"]].float()
        nll, _, gamma, grad = R.ctc_ref(xb.double(), labels, in_len)
        g32 = R.ctc_ref(xb, labels, in_len, dtype=torch.float32)[2]
        gmax = grad.abs().max().item()
        e32 = _maxerr(R.torch_ctc(xb, labels, in_len, torch.float32)[1], grad) / gmax if gmax > 0 else 0.0
        out.append(dict(nll=nll.item(), gamma=gamma, grad=grad, gmax=gmax, e32_gamma=_maxerr(g32, gamma), e32=e32))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name,regime", R.all_ctc_cases())
def test_ctc_edges(dev, name, regime, dtype):
    """avsr_ctc_fwd / avsr_ctc_bwd on the case tables of tests/ctc_loss_ref.py: nll, the occupancies
    gamma and the logits gradient against the fp64 forward-backward; exact zeros for infeasible and
    empty utterances, frames past in_len, states past S and padded columns; no output left unwritten.
    gamma is held to max(3 * e32_gamma, 1e-4) and the fp32 gradient to max(3 * e32, 1e-4) relative
    to the largest reference gradient, where e32_gamma / e32 are the errors of the fp32 reference
    recursion / of torch's fp32 ctc_loss on the same utterance; bf16 gradients to 1e-2.
    Measured on an MI355X, the largest over a case's feasible utterances of |kernel - fp64|, with
    the fp32 reference's own error in brackets (gamma: e32_gamma; dx: e32, both dx figures
    relative to the largest reference gradient):
      case         logits    nll             fp32: gamma            dx                 bf16: gamma           dx
      one-frame    random    1.1 .. 7.9      0       (0)            8.4e-8 (4.7e-8)    0       (0)           2.8e-3
      short        random    7.2 .. 254      6.1e-5 (7.6e-5)        6.1e-5 (6.9e-5)    4.9e-5 (4.9e-5)       2.8e-3
      chunk-edges  random    250 .. 498      8.2e-5 (1.0e-4)        9.7e-5 (1.0e-4)    1.7e-4 (2.1e-4)       2.2e-3
      wide         random    1008 .. 2766    1.5e-3 (1.5e-3)        1.5e-3 (1.4e-3)    1.7e-3 (1.7e-3)       4.2e-3
      two-symbols  random    31 .. 55        8.2e-6 (1.1e-5)        8.3e-6 (9.9e-6)    1.8e-5 (2.2e-5)       2.5e-3
      vocab        random    27 .. 74        3.3e-6 (4.3e-6)        4.0e-6 (4.8e-6)    8.9e-6 (7.8e-6)       2.6e-3
      chunk-edges  match     0.044 .. 0.11   5.8e-8 (5.8e-8)        4.5e-5 (2.9e-7)    5.0e-8 (5.0e-8)       2.5e-3
      wide         match     0.20 .. 0.34    4.2e-8 (3.6e-7)        3.7e-5 (3.8e-7)    4.4e-8 (3.6e-7)       2.2e-3
      chunk-edges  mismatch  553 .. 586      1.8e-4 (2.2e-4)        1.8e-4 (2.3e-4)    2.4e-4 (2.4e-4)       2.1e-3
      wide         mismatch  771 .. 6070     4.1e-3 (4.1e-3)        4.1e-3 (4.1e-3)    4.6e-3 (4.9e-3)       6.7e-3
    nll is within 0.17 of its bound (1e-5 |ref| + 1e-4) everywhere; gamma and the fp32 dx are at
    most 0.45 of theirs, the bf16 dx at most 0.67 (wide / mismatch). The kernel's errors track the
    fp32 reference's: both round lp(t, s) = x - lse to fp32 before the recursion.
    The fp32 dx of the `match` cases is the one figure above e32: there the posterior and the
    occupancy of the planted symbol are both near 1 and the largest gradient is ~5e-3, so an
    absolute 1e-7 in the softmax is 2e-5 of it. Before avsr_ctc_bwd renormalised exp(x - lse) by
    its row sum these cases measured 1.0e-4 .. 1.7e-4 (half an ulp of lse ~ 12 is 5e-7) and
    failed the 1e-4 floor."""
    c = R.CTC_CASES[name]
    T, V, ldx, lddx, utts = c["T"], c["V"], c["ldx"], c["lddx"], c["utts"]
    B = len(utts)
    Lmax = max(1, max(len(l) for l, _ in utts))
    SS = 2 * Lmax + 1
    x = R.case_logits(name, regime, dtype)
    refs = _ctc_refs(name, regime, dtype)
    lab = torch.full((B, Lmax), -1, dtype=torch.int32)
    for b, (l, _) in enumerate(utts):
        lab[b, :len(l)] = torch.tensor(l, dtype=torch.int32)
    xd = x.reshape(B * T, ldx).to(dev)
    assert xd.stride(0) == ldx and (ldx == V or torch.isnan(xd[:, V:]).all())
    lse = ops.row_lse(xd, V, torch.full((B * T,), NAN, device=dev))
    assert torch.isfinite(lse).all()
    alpha = torch.full((B, T, SS), NAN, device=dev)
    gamma = torch.full((B, T, SS), NAN, device=dev)
    nll = torch.full((B,), NAN, device=dev)
    p = ops.ctc_params(xd, B, T, V, lab.to(dev), torch.tensor([len(l) for l, _ in utts], dtype=torch.int32, device=dev),
                       torch.tensor([n for _, n in utts], dtype=torch.int32, device=dev), lse, alpha, gamma, nll)
    ops.ctc_fwd(p)
    dx = torch.full((B * T, lddx), NAN, device=dev, dtype=dtype)
    ops.ctc_bwd(p, torch.tensor([0.7], device=dev), 1.0 / B, dx)
    nll, gamma, dx = nll.cpu(), gamma.cpu(), dx.cpu().float().view(B, T, lddx)
    assert not torch.isnan(nll).any() and not torch.isnan(gamma).any()
    assert not torch.isnan(dx).any()                             # every element written
    assert _zero(dx[:, :, V:])
    scale = 0.7 / B
    bad = []
    for b, (labels, in_len) in enumerate(utts):
        r = refs[b]
        Tb, S = max(0, min(in_len, T)), 2 * len(labels) + 1
        tag = f"{name}/{regime}/{'f32' if dtype == torch.float32 else 'bf16'} utt {b} (L={len(labels)} @{in_len})"
        if not R.feasible(labels, in_len, T):
            assert r["nll"] == 0 and nll[b].item() == 0, tag
            assert _zero(gamma[b]) and _zero(dx[b]), tag
            print(f"{tag}: no path, all outputs exactly 0")
            continue
        assert _zero(gamma[b, Tb:]) and _zero(gamma[b, :, S:]) and _zero(dx[b, Tb:]), tag
        e_nll = abs(nll[b].item() - r["nll"])
        e_gamma = _maxerr(gamma[b, :Tb, :S], r["gamma"][:Tb])
        e_dx = _maxerr(dx[b, :Tb, :V], r["grad"][:Tb] * scale) / (r["gmax"] * scale)
        print(f"{tag}: nll {r['nll']:.6g} err {e_nll:.2g}; gamma err {e_gamma:.2g} (e32_gamma {r['e32_gamma']:.2g}); "
              f"dx err {e_dx:.2g} (e32 {r['e32']:.2g})")
        if not e_nll <= 1e-5 * abs(r["nll"]) + 1e-4:
            bad.append((tag, "nll", e_nll, r["nll"]))
        if not e_gamma <= max(3 * r["e32_gamma"], 1e-4):
            bad.append((tag, "gamma", e_gamma, r["e32_gamma"]))
        if not e_dx < (max(3 * r["e32"], 1e-4) if dtype == torch.float32 else 1e-2):
            bad.append((tag, "dx", e_dx, r["e32"]))
    assert not bad, bad


def test_ctc_fwd_rejects_long_labels(dev):
    """2 * Lmax + 1 > 1024: AVSR_E_SHAPE (1001) from avsr_ctc_fwd, nothing launched or written"""
    B, T, V, ldx, Lmax = 1, 2, 9, 16, 512
    xd = torch.zeros(B * T, ldx, device=dev)
    lse = ops.row_lse(xd, V, torch.empty(B * T, device=dev))
    gamma = torch.full((B, T, 2 * Lmax + 1), NAN, device=dev)
    alpha = torch.full((B, T, 2 * Lmax + 1), NAN, device=dev)
    nll = torch.full((B,), NAN, device=dev)
    p = ops.ctc_params(xd, B, T, V, torch.ones(B, Lmax, dtype=torch.int32, device=dev),
                       torch.tensor([1], dtype=torch.int32, device=dev), torch.tensor([2], dtype=torch.int32, device=dev),
                       lse, alpha, gamma, nll)
    with pytest.raises(L.AvsrLibError, match="1001"):
        ops.ctc_fwd(p)
    torch.cuda.synchronize()
    assert torch.isnan(gamma).all() and torch.isnan(alpha).all() and torch.isnan(nll).all()


# ------------------------------------------------- row_lse, lsm_fwd, lsm_bwd, token_logp
# below, at and just past one 256-thread sweep of each dtype's vector width (4 fp32, 8 bf16)
XENT_V = [2, 5, 8, 9, 1024, 1025, 2048, 2049, 5049]


def _tie_pairs(V):
    """(i, j), i < j, of the two tie rows: next to each other at small V, in different threads
    and sweeps at large V (at 5049, fp32: (3, 4000) = thread 0 sweep 0 / thread 232 sweep 3 and
    (57, 2053) = thread 14 sweep 0 / thread 1 sweep 2, so the later index sits in the lower thread)"""
    if V <= 9:
        return (V - 2, V - 1), (0, 1)
    if V == 5049:
        return (3, 4000), (57, 2053)
    return (3, V - 1), (57, V // 2 + 5)


@functools.lru_cache(maxsize=None)
def _xent_case(V, dtype):
    """8 rows: randn * 2; confident on the target (= V - 1); confident on another column (target 0);
    all + 80; all - 80; all equal (target 0); two tie rows (target = first / second maximum).
    One of the first six rows is ignored (target -1), a different one per V. -> stored x (8, ldx)
    with NaN pads, targets, and the fp64 lse / log-softmax / argmax of the stored values."""
    idx = XENT_V.index(V)
    ldx = (V + 7) // 8 * 8 + (8 if idx % 2 else 0)
    g = torch.Generator().manual_seed(500 + V)
    r = torch.randn(8, V, generator=g)
    tg = torch.randint(0, V, (8,), generator=g)
    x = torch.full((8, ldx), NAN)
    x[0, :V] = r[0] * 2
    x[1, :V] = r[1]; x[1, V - 1] += 20; tg[1] = V - 1
    x[2, :V] = r[2]; x[2, V // 2] += 20; tg[2] = 0
    x[3, :V] = r[3] * 2 + 80
    x[4, :V] = r[4] * 2 - 80
    x[5, :V] = 1.5; tg[5] = 0
    (i6, j6), (i7, j7) = _tie_pairs(V)
    x[6, :V] = r[6] * 2; x[6, i6] = x[6, j6] = 16.0; tg[6] = i6
    x[7, :V] = r[7] * 2; x[7, i7] = x[7, j7] = 16.0; tg[7] = j7
    tg[idx % 6] = -1
    x = x.to(dtype)
    xs = x[:, :V].double()
    return x, tg, torch.logsumexp(xs, 1), torch.log_softmax(xs, 1), xs.argmax(1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("V", XENT_V)
def test_xent_rows(dev, V, dtype):
    """row_lse, lsm_fwd (smoothing 0.1 and 0), token_logp and lsm_bwd on rows of every regime
    against fp64 of the stored values. lse and row_loss: |err| <= 1e-5 * max(1, |ref|) (fp32
    arithmetic: a few ulp in a sum of at most 5049 terms plus one rounding at |lse| ~ 85);
    row_correct is torch.argmax's first-index rule; at smoothing 0 the row loss is bit for bit
    lse - float(x[target]); gradients 1e-5 (fp32) / 1e-2 (bf16) of the largest element."""
    x, tg, lse_ref, logsm, amax = _xent_case(V, dtype)
    ldx, lddx = x.shape[1], x.shape[1] + 8
    ign = tg < 0
    xd, tgd = x.to(dev), tg.to(torch.int32).to(dev)
    assert ldx == V or torch.isnan(xd[:, V:]).all()
    lse0 = ops.row_lse(xd, V, torch.full((8,), NAN, device=dev)).cpu()
    tol = 1e-5 * lse_ref.abs().clamp_min(1)
    assert ((lse0.double() - lse_ref).abs() <= tol).all(), (lse0, lse_ref)
    rc_ref = torch.where(ign, torch.tensor(-1), (amax == tg).long()).to(torch.int32)
    assert rc_ref[6] == 1 and rc_ref[7] == 0                    # the tie rows: first index wins
    xt = x.float()[torch.arange(8), tg.clamp_min(0)]            # float(x[row][target])
    for sm in (0.1, 0.0):
        lse = torch.full((8,), NAN, device=dev); rl = torch.full((8,), NAN, device=dev)
        rc = torch.full((8,), 7, dtype=torch.int32, device=dev)
        ops.lsm_fwd(xd, V, tgd, sm, lse, rl, rc)
        lse, rl, rc = lse.cpu(), rl.cpu(), rc.cpu()
        assert torch.equal(lse, lse0)                            # one row reduction behind both entries
        q = torch.full((8, V), sm / (V - 1), dtype=torch.float64)
        q.scatter_(1, tg.clamp_min(0).unsqueeze(1), 1 - sm)
        kl = (torch.xlogy(q, q) - q * logsm).sum(1).masked_fill(ign, 0)
        err = (rl.double() - kl).abs()
        print(f"V={V} {dtype} sm={sm}: lse err {(lse0.double() - lse_ref).abs().max():.2g}, row_loss err {err.max():.2g}")
        assert (err <= 1e-5 * kl.abs().clamp_min(1)).all(), (rl, kl)
        assert (rl[ign] == 0).all()
        assert torch.equal(rc, rc_ref), (rc, rc_ref)
        if sm == 0.0:
            assert torch.equal(rl[~ign], (lse - xt)[~ign])       # bit for bit
            tlp = ops.token_logp(xd, V, tgd).cpu()
            assert torch.equal(tlp, -rl) and torch.equal(tlp[~ign], (xt - lse)[~ign]) and (tlp[ign] == 0).all()
        dx = torch.full((8, lddx), NAN, device=dev, dtype=dtype)
        ops.lsm_bwd(xd, V, tgd, sm, lse.to(dev), torch.tensor([0.9], device=dev), 1.0 / 3, dx)
        dx = dx.cpu().float()
        assert not torch.isnan(dx).any()
        assert _zero(dx[:, V:]) and _zero(dx[ign])
        gref = (0.9 / 3) * (logsm.exp() - q).masked_fill(ign.unsqueeze(1), 0)
        gerr = _maxerr(dx[:, :V], gref) / gref.abs().max().item()
        assert gerr < (1e-5 if dtype == torch.float32 else 1e-2), gerr


# ---------------------------------------------------------------------------- loss_finalize
def _finalize_ref(nll, rl, rc, mtl, per_token):
    """fp64 {loss, loss_ctc, loss_att, acc} and, per output, the sum of the |terms| it adds up"""
    B = nll.numel()
    nll, rl = nll.double(), rl.double()
    valid = int((rc >= 0).sum()) if rc is not None else 0
    div = max(valid, 1) if per_token else B
    lc, la = nll.sum().item() / B, rl.sum().item() / div
    mc, ma = nll.abs().sum().item() / B, rl.abs().sum().item() / div
    acc = int((rc == 1).sum()) / valid if valid else 0.0
    return [mtl * lc + (1 - mtl) * la, lc, la, acc], [mtl * mc + (1 - mtl) * ma, mc, ma, acc]


def _finalize_check(dev, nll, rl, rc, mtl, per_token):
    out = torch.full((4,), NAN, device=dev)
    ops.loss_finalize(nll.numel(), nll.to(dev), rl.to(dev), None if rc is None else rc.to(dev), mtl, out,
                      att_per_token=per_token)
    ref, mag = _finalize_ref(nll, rl, rc, mtl, per_token)
    for o, r, m in zip(out.cpu().tolist(), ref, mag):
        assert abs(o - r) <= 1e-5 * m + 1e-6, (out, ref)


@pytest.mark.parametrize("mtl", [0.1, 1.0])
@pytest.mark.parametrize("per_token", [False, True])
def test_loss_finalize_strided(dev, per_token, mtl):
    """B = 300 utterances and 1000 rows: both 256-thread loops stride; row_correct mixes -1 / 0 / 1;
    then every row ignored (per token: divides by 1; acc 0)"""
    B, rows = 300, 1000
    g = torch.Generator().manual_seed(6)
    nll = torch.rand(B, generator=g) * 200
    nll[::11] = 0                                               # zero_infinity utterances
    rc = torch.randint(-1, 2, (rows,), generator=g).to(torch.int32)
    rl = (torch.rand(rows, generator=g) * 9).masked_fill(rc < 0, 0)
    _finalize_check(dev, nll, rl, rc, mtl, per_token)
    _finalize_check(dev, nll, torch.zeros(rows), torch.full((rows,), -1, dtype=torch.int32), mtl, per_token)


def test_loss_finalize_without_rows(dev):
    """rows = 0 with row_correct = None (the CTC-only call): loss = mtl * loss_ctc, loss_att = acc = 0;
    att_per_token without row_correct is AVSR_E_ARG (1004) and writes nothing"""
    nll = torch.rand(300, generator=torch.Generator().manual_seed(7)) * 50
    for mtl in (1.0, 0.3):
        _finalize_check(dev, nll, torch.zeros(0), None, mtl, False)
    out = torch.full((4,), NAN, device=dev)
    with pytest.raises(L.AvsrLibError, match="1004"):
        ops.loss_finalize(300, nll.to(dev), torch.zeros(8, device=dev), None, 0.3, out, att_per_token=True)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()

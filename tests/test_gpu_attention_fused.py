"""The one-kernel encoder attention backward (rb::attn_bwd_kernel, option attn_enc_fused = 1)
against the two-kernel path it replaces (option 0: dQ kernel, then dK / dV kernel) on the same
bf16 inputs: dK, dV and delta bit for bit, dQ within the bound test_gpu_attention.py applies
between a bf16 backward and its reference, no worse than the two-kernel dQ against an fp64
reference, nothing written outside the rows of the outputs, and the same bits on every run."""
import pytest
import torch

from avsr_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.0            # exact in bf16
PAD = 4                    # rows past the end of every gradient buffer


def _rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


SHAPES = [
    # B, H, Lq, Lk, klen
    (1, 1, 128, 128, None),                 # four tiles; two ring rounds, the second partial
    (3, 2, 130, 130, None),                 # ragged last tile; grid not a multiple of 8 (XCD remap)
    (3, 2, 200, 200, [200, 129, 64]),       # a whole key block past klen, inactive waves, klen < 128
    (2, 2, 288, 288, None),                 # exactly three rounds: the ring slot is reused once
    (2, 2, 375, 375, [375, 301]),           # the workload's own length
    (1, 2, 384, 384, None),                 # the full image, every wave active
    (1, 2, 160, 352, None),                 # Lq != Lk
    (1, 2, 352, 160, None),
]
MODES = ["nodrop", "hashed", "stored"]


def _reference_dq(q, k, v, dout, B, H, Lq, Lk, klen):
    """fp64 autograd dQ on the bf16 inputs (drop_p = 0)"""
    qr = q.double().cpu().clone().requires_grad_()
    kr, vr = k.double().cpu(), v.double().cpu()
    qh = qr.view(B, Lq, H, 64).transpose(1, 2)
    kh = kr.view(B, Lk, H, 64).transpose(1, 2)
    vh = vr.view(B, Lk, H, 64).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * 0.125
    if klen is not None:
        m = (torch.arange(Lk)[None, :] < torch.tensor(klen)[:, None])[:, None, None, :]
        s = s.masked_fill(~m, float("-inf"))
    out = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B * Lq, H * 64)
    out.backward(dout.double().cpu())
    return qr.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,Lq,Lk,klen", SHAPES)
def test_fused_backward_matches_two_kernel_path(dev, lib_opt, B, H, Lq, Lk, klen, mode):
    assert ops.attn_path(torch.bfloat16, B, H, Lq, Lk, backward=True) == "enc"
    D = H * 64
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(Lq + H)
    if Lq == Lk:
        qkv = torch.randn(B * Lq, 3 * D, generator=g).to(dev, bf)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        q = torch.randn(B * Lq, D, generator=g).to(dev, bf)
        kv = torch.randn(B * Lk, 2 * D, generator=g).to(dev, bf)
        k, v = kv[:, :D], kv[:, D:]
    dout = torch.randn(B * Lq, D, generator=g).to(dev, bf)
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32, device=dev)
    p = 0.0 if mode == "nodrop" else 0.1
    mask = None
    if mode == "stored":
        mask = torch.empty(ops.attn_mask_words(B, H, Lq, Lk), device=dev, dtype=torch.int64)
        ops.attn_dropmask(mask, B=B, H=H, Lq=Lq, Lk=Lk, drop_p=p, seed=99)
    o = torch.empty(B * Lq, D, device=dev, dtype=bf)
    lse = torch.empty(B, H, Lq, device=dev)
    ops.attn_fwd(q, k, v, o, lse, B=B, H=H, Lq=Lq, Lk=Lk, klen=kl, scale=0.125, drop_p=p, seed=99, mask=mask)

    def run(fused):
        lib_opt("attn_enc_fused", fused)
        if Lq == Lk:
            buf = torch.full((B * Lq + PAD, 3 * D), SENTINEL, device=dev, dtype=bf)
            dq, dk, dv = buf[:B * Lq, :D], buf[:B * Lk, D:2 * D], buf[:B * Lk, 2 * D:]
            tails = [buf[B * Lq:]]
        else:
            bq = torch.full((B * Lq + PAD, D), SENTINEL, device=dev, dtype=bf)
            bkv = torch.full((B * Lk + PAD, 2 * D), SENTINEL, device=dev, dtype=bf)
            dq, dk, dv = bq[:B * Lq], bkv[:B * Lk, :D], bkv[:B * Lk, D:]
            tails = [bq[B * Lq:], bkv[B * Lk:]]
        delta = torch.full((B, H, Lq), SENTINEL, device=dev)
        ops.attn_bwd(dout, q, k, v, o, lse, None, dk, dv, delta, B=B, H=H, Lq=Lq, Lk=Lk, klen=kl, scale=0.125,
                     drop_p=p, seed=99, dq=dq, mask=mask)
        for t in tails:                                  # nothing past the rows of an output
            assert bool((t == SENTINEL).all())
        return dq, dk, dv, delta

    dq1, dk1, dv1, de1 = run(1)
    dq1b, dk1b, dv1b, de1b = run(1)
    dq0, dk0, dv0, de0 = run(0)
    for t in (dq1, dk1, dv1, de1, dq0, dk0, dv0):
        assert bool(torch.isfinite(t.float()).all())
    # no atomics, a fixed summation order
    assert torch.equal(dq1, dq1b) and torch.equal(dk1, dk1b) and torch.equal(dv1, dv1b) and torch.equal(de1, de1b)
    # dK, dV, delta: the dK / dV kernel's arithmetic and order, the dQ kernel's delta
    assert torch.equal(dk1, dk0)
    assert torch.equal(dv1, dv0)
    assert torch.equal(de1, de0)
    # dQ is built from the dK / dV pass's dS (one rounding per element away from the dQ kernel's)
    between = _rel(dq1, dq0)
    print(f"\nfused-vs-split dq rel B{B} H{H} Lq{Lq} Lk{Lk} {mode}: {between:.3e}")
    assert between < 3e-2
    if mode == "nodrop":
        ref = _reference_dq(q, k, v, dout, B, H, Lq, Lk, klen)
        e1, e0 = _rel(dq1, ref), _rel(dq0, ref)
        print(f"dq error vs fp64 B{B} H{H} Lq{Lq} Lk{Lk}: fused {e1:.3e} two-kernel {e0:.3e}")
        assert e1 <= 1.25 * e0

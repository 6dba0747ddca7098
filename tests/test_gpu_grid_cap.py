"""The grid-capped BatchNorm, pooling and elementwise kernels above their grid cap, vs torch fp64.

avsr_grid / bn_grid cap a launch at `cap` blocks of 256 threads; with more work than
cap * 256 items the kernels' grid-stride code runs: a second (third, ...) vector per thread,
the 2-wide / 4-wide iterations with dead slots and clamped loads, a channel group fixed per
thread across strides, multiply-shift index decomposition with dividends in the millions.
S = 2048 * 256 = 524,288 is the default capped stride. Every case here has a partial last
block (wherever the shape allows one), writes into NaN-filled (uint8: 255-filled) outputs
that sit in front of a guard region, and asserts that nothing is left unwritten and that the
guard is untouched.

Audit of every avsr_grid( / bn_grid( call site (items = work items of one launch; C2 = one
training step at B = 16, T = 375, 6000 frames, bf16; beam-5 = 16 utterances x 5 hypotheses):

call site                                  cap (items)   workload (items)              covering test
batchnorm.hip bn_act_fwd                   524,288       23.2 M (C2 stage 1)           test_bn_chain_* (here)
batchnorm.hip bn_act_bwd_reduce            524,288       23.2 M                        test_bn_chain_* (here)
batchnorm.hip bn_bwd_apply                 524,288       23.2 M                        test_bn_chain_* (here)
pool.hip stem_pool_fwd (2x2 blocks)        524,288       5.8 M                         test_stem_pool_fwd_above_cap (here)
pool.hip stem_pool_bwd_apply (2x2)         524,288       23.2 M                        test_stem_bwd_apply_above_cap[block12] (here)
pool.hip stem_pool_bwd_apply (pixel)       524,288       odd frame sizes only          test_stem_bwd_apply_above_cap[pixel*] (here)
pool.hip avgpool_fwd                       524,288       384,000 (fp32: 768,000)       test_avgpool_above_cap (here)
pool.hip avgpool_bwd                       524,288       3.46 M                        test_avgpool_above_cap (here)
elementwise.hip mask_rows                  524,288       768,000 (16 x 375 x 1024)     test_mask_rows_above_cap (here)
elementwise.hip embed_fwd                  524,288       token rows x 128: below the   below the cap; test_gpu_loss_misc (direct)
                                                         cap up to 4096 rows (C2: 16 x
                                                         label length; beam-5: 10,240)
elementwise.hip audio_pack                 524,288       624,000 (16 x 104 x 375)      test_audio_pack_above_cap (here)
param.hip weightnorm_fwd (wn_apply)        524,288       8.4 M (1024 x 128 x 64)       test_gpu_loss_misc::test_weightnorm[1024-128-64]
param.hip weightnorm_bwd (wn_bwd)          524,288       8.4 M                         test_gpu_loss_misc::test_weightnorm[1024-128-64]
param.hip sumsq                            262,144 x4    the gradient arena, 10^8      test_sumsq_above_cap (here; the existing
                                                                                       3,000,003-element call feeds only the clip)
param.hip adamw                            1,048,576 x4  the arena in slices; the      test_gpu_loss_misc::
                                           or max_blocks overlapped update caps at     test_adamw_grid_cap_bit_identical (caps 64, 512
                                                         max_blocks                    against the uncapped grid, bit for bit)
frontend.hip video_normalize               1,048,576 x4  11.6 M (6000 x 88 x 22)       test_video_normalize_above_cap (here)
augment.hip  rgb_to_gray                   1,048,576     3.46 M (375 x 96 x 96)        test_rgb_to_gray_above_cap (here)
gemm.hip   slab_reduce                     1,048,576 x4  <= 1,048,576 (4096 x 1024     at the cap, not above; test_gpu_gemm::
                                           per batch     weight gradient)              test_gemm_layouts_bf16[6000-1024-512-2] is above
beam.hip beam_kv_put                       262,144       10,240 (80 x 1024 / 8)        below the cap at beam-5 (above it only for fp32 with
                                                                                       > 1024 rows): test_beam_kv_put_above_cap (here)
beam.hip gather_rows   (16-byte words)     524,288       <= 60,000 (80 rows x 750 x 4  below the cap at beam-5 (above it from 700 rows of
beam.hip gather_rows   (4-byte words)      524,288       bytes)                        375 frames): test_gather_rows_above_cap (here)
attention.hip attn_bwd_prep                524,288       96,000 (16 x 375 x 16)        below the cap; test_gpu_attention (f32 / tiled backward)
conv.hip   stem weight-grad reduce         262,144 x4    6,272 x4 (64 x 392)           below the cap; test_gpu_conv (stem weight gradient)
conv.hip   conv weight-grad slab reduce    262,144 x4    589,824 x4 (3 x 3 x 512 x     test_gpu_conv (weight gradient at 3 x 3 x 512 x 512)
                                                         512)
common.h   avsr_grid itself / norm.h bn_grid: the helpers.
"""
import math

import pytest
import torch

from avsr_amd import frontend, ops

pytestmark = pytest.mark.gpu

S = 2048 * 256            # vectors (items) one capped launch covers per grid stride
GUARD = 4096              # elements behind every output
GUARD_VALUE = 7.0
BF, F32 = torch.bfloat16, torch.float32


def _rel(a, b):
    a = a.detach().double(); b = b.detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _tol(dtype, f32=2e-5, b16=2e-2):
    return f32 if dtype == F32 else b16


def _ve(dtype):
    return 8 if dtype == BF else 4


def _guarded(shape, dtype, dev, fill=None):
    """an output of `shape` filled with NaN (uint8: 255) followed by GUARD elements of GUARD_VALUE"""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), GUARD_VALUE, device=dev, dtype=dtype)
    if fill is None:
        fill = 255 if dtype == torch.uint8 else float("nan")
    buf[:n] = fill
    return buf[:n].view(shape), buf[n:]


def _assert_written(out, guard, name):
    torch.cuda.synchronize()
    assert bool((guard == GUARD_VALUE).all()), f"{name}: written past the end"
    if out.dtype == torch.uint8:
        assert not bool((out == 255).any()), f"{name}: elements left unwritten"
    else:
        assert not bool(torch.isnan(out).any()), f"{name}: elements left unwritten"


def _rows(regime, cpv):
    """M = 37 (mod 64) with M * cpv ~ regime * S: M is odd and cpv <= 128, so M * cpv is no multiple of 256"""
    m = int(regime * S / cpv)
    m = m - m % 64 + 37
    assert (m * cpv) % 256
    return m


# ------------------------------------------------------------------ A. BatchNorm + PReLU chain

_PAIRS = [(BF, 64), (F32, 512)]
BN_CASES = [(dt, C, 1.5, "plain") for dt in (BF, F32) for C in (64, 128, 256, 512)]
BN_CASES += [(dt, C, reg, mode) for dt, C in _PAIRS for reg in (1.5, 2.5, 4.5)
             for mode in ("plain", "identity", "downsample") if (reg, mode) != (1.5, "plain")]
_BN_IDS = [f"{'bf16' if dt == BF else 'fp32'}-{C}-{reg}S-{mode}" for dt, C, reg, mode in BN_CASES]


def _bn_reference(h, r, dy, st, st2, a, mode):
    """fp64 formulas of the chain from the operands as stored: z, y, dz and the four column sums"""
    dbl = lambda t: t.double()
    h, r, dy, a = dbl(h), dbl(r), dbl(dy), dbl(a)
    z = h * dbl(st.scale) + dbl(st.shift)
    if mode == "identity":
        z = z + r
    elif mode == "downsample":
        z = z + r * dbl(st2.scale) + dbl(st2.shift)
    pos = z > 0
    y = torch.where(pos, z, z * a)
    dz = torch.where(pos, dy, dy * a)
    t0 = dz
    t1 = dz * (h - dbl(st.mean)) * dbl(st.invstd)
    t2 = dz * (r - dbl(st2.mean)) * dbl(st2.invstd) if mode == "downsample" else torch.zeros_like(dz)
    t3 = torch.where(pos, torch.zeros_like(dy), dy * z)
    return z, y, dz, (t0, t1, t2, t3)


def _bn_res_args(mode, r, st2):
    return dict(res=None if mode == "plain" else r, st2=st2 if mode == "downsample" else None)


@pytest.mark.parametrize("dtype,C,regime,mode", BN_CASES, ids=_BN_IDS)
def test_bn_chain_elementwise(dev, dtype, C, regime, mode):
    """y, dz, dh, dh2 of bn_act_fwd / bn_act_bwd_reduce / bn_bwd_apply with random normal data
    above the cap: 1.5 S (a second vector for some threads: ok = {1, 1 or 0, 0, 0}), 2.5 S (a
    second iteration of the 2-wide loops with `two` false), 4.5 S (a second iteration of the
    4-wide apply with one live slot). The apply gets the reference dz and sums, so its check
    does not depend on the reduction; once more with beta_acc = 1 into a non-zero dh."""
    cpv = C // _ve(dtype)
    M = _rows(regime, cpv)
    g = torch.Generator(device=dev).manual_seed(1000 * C + int(10 * regime))
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    h = (rn(M, C) * 1.5 + 0.3).to(dtype)
    r = (rn(M, C) * 0.7 - 0.2).to(dtype)
    dy = rn(M, C).to(dtype)
    a = 0.25 + 0.05 * rn(C)

    def state():
        st = ops.BnState(C, dev)
        st.mean.copy_(0.1 * rn(C)); st.invstd.copy_(0.5 + torch.rand(C, generator=g, device=dev))
        st.scale.copy_(1 + 0.2 * rn(C)); st.shift.copy_(0.2 * rn(C))
        return st
    st, st2 = state(), state()
    z, y_ref, dz_ref, terms = _bn_reference(h, r, dy, st, st2, a, mode)
    res = _bn_res_args(mode, r, st2)

    y, yg = _guarded((M, C), dtype, dev)
    ops.bn_act_fwd(h, st, a, y, **res)
    _assert_written(y, yg, "y")
    assert _rel(y, y_ref) < _tol(dtype, 1e-5)

    tol = _tol(dtype, 1e-4, 3e-2)
    dz, dzg = _guarded((M, C), dtype, dev)
    grads = [torch.zeros(C, device=dev) for _ in range(5)]
    ops.bn_act_bwd_reduce(dy, h, st, a, dz=dz, dprelu=grads[4], dgamma=grads[0], dbeta=grads[1],
                          dgamma2=grads[2] if mode == "downsample" else None,
                          dbeta2=grads[3] if mode == "downsample" else None, **res)
    _assert_written(dz, dzg, "dz")
    # dz jumps at z = 0: where the fp64 z lies within fp32 rounding of 0 (|z| <= 14 here, so
    # 1e-4 is 100 x the fp32 error of z) the kernel's fp32 z may take either branch
    alt = torch.where(z > 0, dy.double() * a.double(), dy.double())
    err = (dz.double() - dz_ref).abs()
    err = torch.where(z.abs() < 1e-4, torch.minimum(err, (dz.double() - alt).abs()), err)
    assert (err.max() / dz_ref.abs().max()).item() < tol

    sums = torch.stack([t.sum(0) for t in terms[:3]], 1).float().contiguous()        # (C, 3), reference
    dz_in = dz_ref.to(dtype)
    S0, S1, S2 = (sums[:, q].double() for q in range(3))
    xh = (h.double() - st.mean.double()) * st.invstd.double()
    dh_ref = st.scale.double() * (dz_in.double() - S0 / M - xh * S1 / M)
    dh, dhg = _guarded((M, C), dtype, dev)
    dh2 = dh2g = dh2_ref = None
    if mode == "downsample":
        dh2, dh2g = _guarded((M, C), dtype, dev)
        xh2 = (r.double() - st2.mean.double()) * st2.invstd.double()
        dh2_ref = st2.scale.double() * (dz_in.double() - S0 / M - xh2 * S2 / M)
    ops.bn_bwd_apply(dz_in, h, st, sums, dh, dh2=dh2, **res)
    _assert_written(dh, dhg, "dh")
    assert _rel(dh, dh_ref) < tol
    if dh2 is not None:
        _assert_written(dh2, dh2g, "dh2")
        assert _rel(dh2, dh2_ref) < tol

    old = rn(M, C).to(dtype)
    dha, dhag = _guarded((M, C), dtype, dev)
    dha.copy_(old)
    dh2a = dh2ag = None
    if mode == "downsample":
        dh2a, dh2ag = _guarded((M, C), dtype, dev)
    ops.bn_bwd_apply(dz_in, h, st, sums, dha, dh2=dh2a, beta_acc=1.0, **res)
    _assert_written(dha, dhag, "dh (beta_acc = 1)")
    assert _rel(dha, old.double() + dh_ref) < tol
    if dh2a is not None:
        _assert_written(dh2a, dh2ag, "dh2 (beta_acc = 1)")
        assert torch.equal(dh2a, dh2)


@pytest.mark.parametrize("dtype,C,regime,mode", BN_CASES, ids=_BN_IDS)
def test_bn_chain_exact_sums(dev, dtype, C, regime, mode):
    """The reduction's column sums and the parameter gradients, exactly. dy, h - mean and
    res - mean2 are integers in [-2, 2], mean and shift integers in [-1, 1], scale and invstd in
    {0.5, 1, 2}, PReLU weights in {0.25, 0.5}: exact in bf16, every product exact in fp32, and,
    as long as a channel's sum of |term| stays below 2^24 units (asserted on the reference), so
    is every partial sum in any order. One dropped or doubled row then changes the result."""
    cpv = C // _ve(dtype)
    M = _rows(regime, cpv)
    g = torch.Generator(device=dev).manual_seed(77 * C + int(10 * regime))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=dev).float()

    def state():
        st = ops.BnState(C, dev)
        st.mean.copy_(ri(-1, 1, C)); st.shift.copy_(ri(-1, 1, C))
        st.scale.copy_(2.0 ** ri(-1, 1, C)); st.invstd.copy_(2.0 ** ri(-1, 1, C))
        return st
    st, st2 = state(), state()
    a = 2.0 ** -ri(1, 2, C)
    h = (st.mean + ri(-2, 2, M, C)).to(dtype)
    r = (st2.mean + ri(-2, 2, M, C)).to(dtype)
    dy = ri(-2, 2, M, C).to(dtype)
    z, y_ref, dz_ref, terms = _bn_reference(h, r, dy, st, st2, a, mode)
    # smallest unit of each sum's terms: dz in quarters; x invstd >= 0.5; dy * z in halves
    for t, unit in zip(terms, (0.25, 0.125, 0.125, 0.5)):
        assert bool((t / unit == (t / unit).round()).all())
        assert (t.abs().sum(0).max() / unit).item() < 2 ** 24
    res = _bn_res_args(mode, r, st2)

    y, yg = _guarded((M, C), dtype, dev)
    ops.bn_act_fwd(h, st, a, y, **res)
    _assert_written(y, yg, "y")
    assert torch.equal(y, y_ref.to(dtype))

    dz, dzg = _guarded((M, C), dtype, dev)
    sums = torch.full((C, 3), float("nan"), device=dev)
    grads = [torch.zeros(C, device=dev) for _ in range(5)]        # dgamma, dbeta, dgamma2, dbeta2, dprelu
    ds = mode == "downsample"
    ops.bn_act_bwd_reduce(dy, h, st, a, dz=dz, sums=sums, dprelu=grads[4], dgamma=grads[0], dbeta=grads[1],
                          dgamma2=grads[2] if ds else None, dbeta2=grads[3] if ds else None, **res)
    _assert_written(dz, dzg, "dz")
    assert torch.equal(dz, dz_ref.to(dtype))
    want = [t.sum(0).float() for t in terms]
    for q in range(3):
        assert torch.equal(sums[:, q], want[q]), f"sums[:, {q}]"
    assert torch.equal(grads[1], want[0]), "dbeta"
    assert torch.equal(grads[0], want[1]), "dgamma"
    assert torch.equal(grads[4], want[3]), "dprelu"
    if ds:
        assert torch.equal(grads[3], want[0]), "dbeta2"
        assert torch.equal(grads[2], want[2]), "dgamma2"


# ------------------------------------------------------------------ B. stem max-pool, C = 64

def _stem_state(C, dev, g):
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    st = ops.BnState(C, dev)
    st.mean.copy_(0.1 * rn(C)); st.invstd.copy_(0.5 + torch.rand(C, generator=g, device=dev))
    st.scale.copy_(1 + 0.2 * rn(C)); st.shift.copy_(0.2 * rn(C))
    return st, 0.25 + 0.05 * rn(C)


def _pool_ref(h, st, a, chunk=512):
    """fp64 maxpool3x3 s2 p1 of prelu(h * scale + shift) over NHWC h: (y, argmax uint8 = the
    first maximum in row-major window order), image chunks"""
    n, H, W, C = h.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    sc, sh, ad = st.scale.double(), st.shift.double(), a.double()
    ys, qs = [], []
    for i in range(0, n, chunk):
        z = h[i:i + chunk].double() * sc + sh
        z = torch.where(z > 0, z, z * ad)
        zp = torch.full((z.shape[0], H + 2, W + 2, C), float("-inf"), device=h.device, dtype=torch.float64)
        zp[:, 1:H + 1, 1:W + 1] = z
        win = torch.stack([zp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)])
        y = win.amax(0)
        ys.append(y)
        qs.append((win == y).int().argmax(0).to(torch.uint8))     # argmax: the first of equal maxima
    return torch.cat(ys), torch.cat(qs)


def _pool_images(dtype, hw, regime):
    """an odd image count with nimg * hw * cpv ~ regime * S (odd: the last block is partial,
    except where one image is whole blocks: 12 x 12 pixels of 16 fp32 vectors)"""
    cpv = 64 // _ve(dtype)
    n = int(regime * S / (hw * cpv)) | 1
    assert (n * hw * cpv) % 256 or (hw * cpv) % 256 == 0
    assert n <= 65535
    return n


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_stem_pool_fwd_above_cap(dev, dtype, lib_opt):
    """stem_pool_fwd on 12 x 12 images (Ho = Wo = 6: the 2x2-block kernel divides its work
    index by 3) with 1.25 S work items; block kernel and per-window kernel agree bit for bit."""
    C, H, W = 64, 12, 12
    n = _pool_images(dtype, 9, 1.25)
    g = torch.Generator(device=dev).manual_seed(12)
    h = torch.randn(n, H, W, C, generator=g, device=dev).to(dtype)
    st, a = _stem_state(C, dev, g)
    fw = []
    for opt in (1, 0):
        lib_opt("stem_pool_2x2", opt)
        y, yg = _guarded((n, 6, 6, C), dtype, dev)
        am, amg = _guarded((n, 6, 6, C), torch.uint8, dev)
        hmax, hg = _guarded((n, 6, 6, C), dtype, dev)
        ops.stem_pool_fwd(h, n, H, W, st, a, y, am, hmax=hmax)
        for t, tg, name in ((y, yg, "y"), (am, amg, "argmax"), (hmax, hg, "hmax")):
            _assert_written(t, tg, f"{name} (stem_pool_2x2 = {opt})")
        fw.append((y, am, hmax))
    for t1, t0 in zip(*fw):
        assert torch.equal(t1, t0)
    y, am, hmax = fw[0]
    y_ref, _ = _pool_ref(h, st, a)
    assert _rel(y, y_ref) < _tol(dtype, 1e-5)
    # hmax = h at the recorded argmax window position, and y = prelu(bn(hmax))
    assert int(am.max()) < 9
    q = am.long()
    ar = lambda k, *shape: torch.arange(k, device=dev).view(*shape)
    ih = 2 * ar(6, 1, 6, 1, 1) - 1 + q // 3
    iw = 2 * ar(6, 1, 1, 6, 1) - 1 + q % 3
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all())
    pick = h[ar(n, n, 1, 1, 1), ih, iw, ar(C, 1, 1, 1, C)]
    assert torch.equal(pick, hmax)
    zm = hmax.double() * st.scale.double() + st.shift.double()
    assert _rel(y, torch.where(zm > 0, zm, zm * a.double())) < _tol(dtype, 1e-5)


@pytest.mark.parametrize("regime", [1.5, 2.5])
@pytest.mark.parametrize("kind", ["block12", "pixel12", "pixel97"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_stem_bwd_apply_above_cap(dev, dtype, kind, regime, lib_opt):
    """stem_pool_bwd_apply vs fp64 with reference sums: the 2x2-block kernel at 12 x 12
    (block12: regime x S blocks), the per-pixel kernel at 12 x 12 with the block kernel switched
    off and at 9 x 7 (regime x S pixels; 1.5 S: a second vector for some threads, 2.5 S: a
    second 2-wide iteration with `two` false). At 12 x 12 the two kernels agree."""
    C = 64
    H, W = (9, 7) if kind == "pixel97" else (12, 12)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    n = _pool_images(dtype, Ho * Wo if kind == "block12" else H * W, regime)
    g = torch.Generator(device=dev).manual_seed(H * W + int(10 * regime))
    h = torch.randn(n, H, W, C, generator=g, device=dev).to(dtype)
    st, a = _stem_state(C, dev, g)
    dzp = torch.randn(n, Ho, Wo, C, generator=g, device=dev).to(dtype)
    _, am = _pool_ref(h, st, a)
    # reference: dz[p] = sum of dzp[o] over the windows o whose argmax is p
    d = dzp.double()
    pad = torch.zeros(n, H + 2, W + 2, C, device=dev, dtype=torch.float64)
    for q in range(9):
        kh, kw = q // 3, q % 3
        pad[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += torch.where(am == q, d, torch.zeros_like(d))
    dz = pad[:, 1:H + 1, 1:W + 1]
    for edge in (pad[:, 0], pad[:, H + 1], pad[:, :, 0], pad[:, :, W + 1]):   # no argmax points outside the image
        assert not bool(edge.any())
    # sums over the pooled grid with h at the argmax (what the stem's reduction hands the apply)
    q = am.long()
    ar = lambda k, *shape: torch.arange(k, device=dev).view(*shape)
    hm = h[ar(n, n, 1, 1, 1), 2 * ar(Ho, 1, Ho, 1, 1) - 1 + q // 3, 2 * ar(Wo, 1, 1, Wo, 1) - 1 + q % 3,
           ar(C, 1, 1, 1, C)].double()
    mean, invstd, scale = st.mean.double(), st.invstd.double(), st.scale.double()
    sums = torch.stack([d.sum((0, 1, 2)), (d * (hm - mean) * invstd).sum((0, 1, 2)), torch.zeros_like(mean)], 1)
    sums = sums.float().contiguous()
    Mt = n * H * W
    dh_ref = scale * (dz - sums[:, 0].double() / Mt - (h.double() - mean) * invstd * sums[:, 1].double() / Mt)

    def run(opt):
        lib_opt("stem_pool_2x2", opt)
        dh, dhg = _guarded((n, H, W, C), dtype, dev)
        ops.stem_pool_bwd_apply(dzp, am, h, n, H, W, st, sums, dh)
        _assert_written(dh, dhg, f"dh (stem_pool_2x2 = {opt})")
        return dh
    tol = _tol(dtype, 1e-4, 3e-2)
    dh = run(0 if kind == "pixel12" else 1)
    assert _rel(dh, dh_ref) < tol
    if kind != "pixel97":
        other = run(1 if kind == "pixel12" else 0)
        assert _rel(other, dh_ref) < tol
        assert _rel(dh, other) < (1e-6 if dtype == F32 else 8e-3)


# ------------------------------------------------------------------ C. average pool

@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_avgpool_above_cap(dev, dtype):
    """avgpool_fwd at nimg * C / VE ~ 1.5 S and avgpool_bwd at nimg * P * C / VE ~ 2.5 S
    (P = 9, C = 512). fp32 within 1e-6; bf16 within one rounding of the output (2^-8 of the
    reference maximum)."""
    P, C = 9, 512
    cpv = C // _ve(dtype)
    tol = 1e-6 if dtype == F32 else 2.0 ** -8
    g = torch.Generator(device=dev).manual_seed(9)
    n = _rows(1.5, cpv)
    x = torch.randn(n, P, C, generator=g, device=dev).to(dtype)
    y, yg = _guarded((n, C), dtype, dev)
    ops.avgpool_fwd(x, n, P, C, y)
    _assert_written(y, yg, "y")
    assert _rel(y, x.double().sum(1) / P) < tol
    n = _rows(2.5, P * cpv)
    assert (n * P * cpv) % 256
    dy = torch.randn(n, C, generator=g, device=dev).to(dtype)
    dx, dxg = _guarded((n, P, C), dtype, dev)
    ops.avgpool_bwd(dy, n, P, C, dx)
    _assert_written(dx, dxg, "dx")
    assert _rel(dx, (dy.double() / P)[:, None, :].expand(n, P, C)) < tol


# ------------------------------------------------------------------ D. the other capped launches

@pytest.mark.parametrize("dtype,N", [(BF, 1024), (F32, 1000)], ids=["bf16", "fp32"])
def test_mask_rows_above_cap(dev, dtype, N):
    """mask_rows at 15 x 409 rows (the C2 shape is 16 x 375 x 1024 bf16; fp32 rows of 1024 are
    whole blocks, so 1000 there): rows past each length zeroed, everything else untouched, bit
    for bit"""
    B, T = 15, 409
    nv = B * T * N // _ve(dtype)
    assert nv > S and nv % 256
    g = torch.Generator(device=dev).manual_seed(4)
    x, xg = _guarded((B * T, N), dtype, dev, fill=0.0)
    x0 = torch.randn(B * T, N, generator=g, device=dev).to(dtype)
    x.copy_(x0)
    lens = torch.randint(0, T + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    lens[0], lens[1] = T, 0
    ops.mask_rows(x, B, T, lens)
    _assert_written(x, xg, "x")
    keep = (torch.arange(T, device=dev)[None, :] < lens[:, None]).reshape(B * T, 1)
    assert torch.equal(x, torch.where(keep, x0, torch.zeros_like(x0)))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_audio_pack_above_cap(dev, dtype):
    """audio_pack (B, F, T) fp32 -> (B*T, F) at 20 x 104 x 375 items (C2: 16 x 104 x 375): a
    transpose and one cast"""
    B, Fq, T = 20, 104, 375
    assert B * Fq * T > S and (B * Fq * T) % 256
    a = torch.randn(B, Fq, T, generator=torch.Generator(device=dev).manual_seed(6), device=dev)
    out, og = _guarded((B * T, Fq), dtype, dev)
    ops.audio_pack(a, out)
    _assert_written(out, og, "out")
    assert torch.equal(out, a.transpose(1, 2).reshape(B * T, Fq).to(dtype))


@pytest.mark.parametrize("cols,n", [(750, 1049), (752, 4181)], ids=["4-byte", "16-byte"])
def test_gather_rows_above_cap(dev, cols, n):
    """gather_rows dst[i] = src[idx[i]] at 1.5 S words: rows of 750 floats (3000 bytes: the
    4-byte path, the CTC prefix state of 375 frames) and of 752 floats (188 16-byte words)"""
    words = n * (cols if cols % 4 else cols // 4)
    assert words > S and words % 256
    g = torch.Generator(device=dev).manual_seed(cols)
    src = torch.randn(500, cols, generator=g, device=dev)
    idx = torch.randint(0, 500, (n,), generator=g, device=dev, dtype=torch.int32)
    dst, dg = _guarded((n, cols), F32, dev)
    ops.gather_rows(src, dst, idx, groups=1, n=n, row_bytes=cols * 4, src_gstride=0, src_rstride=cols * 4,
                    dst_gstride=0, dst_rstride=cols * 4)
    _assert_written(dst, dg, "dst")
    assert torch.equal(dst, src[idx.long()])


def test_beam_kv_put_above_cap(dev):
    """beam_kv_put at 1.5 x its 1024-block cap (fp32, 1573 rows of 250 vectors): cache rows
    pos * R + r take qkv[r][D:2D] / qkv[r][2D:3D], the other position stays untouched"""
    R, D, p = 1573, 1000, 1
    assert R * D // 4 > 1024 * 256 and (R * D // 4) % 256
    g = torch.Generator(device=dev).manual_seed(33)
    qkv = torch.randn(R, 3 * D + 8, generator=g, device=dev)
    ck, ckg = _guarded((2 * R, D), F32, dev, fill=-5.0)
    cv, cvg = _guarded((2 * R, D), F32, dev, fill=-6.0)
    ck[p * R:], cv[p * R:] = float("nan"), float("nan")
    ops.beam_kv_put(qkv, ck, cv, torch.tensor([p], dtype=torch.int32, device=dev), R, D)
    _assert_written(ck, ckg, "cache_k")
    _assert_written(cv, cvg, "cache_v")
    assert torch.equal(ck[p * R:], qkv[:, D:2 * D]) and torch.equal(cv[p * R:], qkv[:, 2 * D:3 * D])
    assert bool((ck[:p * R] == -5.0).all()) and bool((cv[:p * R] == -6.0).all())


def test_sumsq_above_cap(dev):
    """sumsq over 1.5 x its 1024-block cap of float4 plus a 3-element tail, accumulated onto a
    non-zero total; integer inputs in [-2, 2] make every partial sum exact in any order"""
    n = 1024 * 256 * 4 * 3 // 2 + 139
    assert n % 4 == 3 and (n // 4) % 256
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randint(-2, 3, (n,), generator=g, device=dev).float()
    want = float((x.double() ** 2).sum()) + 5.0
    assert want < 2 ** 24
    out = torch.full((1,), 5.0, device=dev)
    ops.sumsq(x, out)
    assert out.item() == want


def test_video_normalize_above_cap(dev):
    """video_normalize at 1.5 x its 4096-block cap of float4 (3 x 271 frames; a C2 batch is 7 x
    the cap), crop at an off-centre offset; the existing test's 1e-5"""
    B, T, H, W, crop, oy, ox = 3, 271, 96, 96, 88, 5, 3
    total4 = B * T * crop * crop // 4
    assert total4 > 4096 * 256 and total4 % 256
    g = torch.Generator(device=dev).manual_seed(2)
    fr = torch.randint(0, 256, (B, T, H, W), generator=g, device=dev, dtype=torch.uint8)
    out, og = _guarded((B, 1, T, crop, crop), F32, dev)
    frontend.video_transform(fr, offsets=(oy, ox), out=out)
    _assert_written(out, og, "out")
    ref = ((fr[:, :, oy:oy + crop, ox:ox + crop].double() / 255.0 - 0.421) / 0.165)[:, None]
    assert (out.double() - ref).abs().max().item() < 1e-5


def test_rgb_to_gray_above_cap(dev):
    """rgb_to_gray at 1.5 x its 4096-block cap of pixels (one 375-frame clip is 3.3 x the
    cap): the fixed-point formula in integers, bit for bit"""
    n = 4096 * 256 * 3 // 2 + 137
    assert n % 256
    g = torch.Generator(device=dev).manual_seed(4)
    rgb = torch.randint(0, 256, (n, 3), generator=g, device=dev, dtype=torch.uint8)
    got = frontend.rgb_to_gray(rgb)
    torch.cuda.synchronize()
    c = rgb.long()
    ref = (c[:, 0] * 4899 + c[:, 1] * 9617 + c[:, 2] * 1868 + 8192) >> 14
    assert torch.equal(got.long(), ref)

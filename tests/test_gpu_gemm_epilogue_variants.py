"""Compile-time epilogue variants of the bf16 GEMM core (gemm_core.h EV_*: the two 192-row tile
configurations carry them) against the generic run-time epilogue, which the 128x128 tile always
runs. Every tile configuration accumulates an output element over the same K order and a variant
keeps the generic epilogue's operations and their order, so the stored tensors must be equal bit
for bit. The fused bias gradient sums per-row-tile partials, so a different tile height
re-associates an fp32 sum of at most M terms: 1e-5 relative, as test_tile_configs_bit_identical.

Shape: M = 1700, N = 1160: ragged in both directions on 192x128 and 128x128 tiles, N % 8 == 0 (a
variant's condition), more than one tile each way. K = 200 ends in a ragged K-tile."""
import pytest
import torch

from avsr_amd import ops, _lib as L

pytestmark = pytest.mark.gpu

M, N, K = 1700, 1160, 200
LAYOUTS = {"fwd": (True, True), "dgrad": (True, False)}     # (a_kmajor, b_kmajor) of the encoder's GEMMs
VARIANTS = ["plain", "bias", "bias_res", "bias_res_drop", "bias_gelu_drop_preact", "gate_gelu_drop",
            "gate_gelu_drop_colsum"]


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


def _inputs(dev, layout, n=N, batch=1):
    ak, bk = LAYOUTS[layout]
    g = torch.Generator().manual_seed(n + batch)
    A = torch.randn(batch, M, K, generator=g).to(dev, torch.bfloat16)
    B = (torch.randn(batch, n, K, generator=g) if bk else torch.randn(batch, K, n, generator=g))
    B = (B * K ** -0.5).to(dev, torch.bfloat16)
    t = dict(bias=torch.randn(n, generator=g).to(dev),
             res=torch.randn(batch, M, n, generator=g).to(dev, torch.bfloat16),
             gate=torch.randn(batch, M, n, generator=g).to(dev, torch.bfloat16))
    return A, B, ak, bk, t


def _launch(dev, inp, variant, out_dtype=torch.bfloat16, n=N, ldc=None, batch=1, c_off=0):
    """one launch of `variant`; returns every tensor it writes"""
    A, B, ak, bk, t = inp
    ldc = ldc or n
    buf = torch.zeros(batch * M * ldc + c_off, device=dev, dtype=out_dtype)
    C = buf[c_off:].view(batch, M, ldc)
    kw = dict(M=M, N=n, K=K, a_kmajor=ak, b_kmajor=bk, lda=K, ldb=B.stride(1), ldc=ldc, ldr=n, batch=batch,
              strideA=A.stride(0), strideB=B.stride(0), strideC=M * ldc, strideR=M * n)
    outs = [C]
    if variant.startswith("bias"):
        kw["bias"] = t["bias"]
    if variant.startswith("bias_res"):
        kw["res"] = t["res"]
        if variant.endswith("drop"):
            kw.update(drop_p=0.1, seed=7)
    if variant == "bias_gelu_drop_preact":
        h = torch.zeros(batch, M, ldc, device=dev, dtype=torch.bfloat16)
        kw.update(act=L.ACT_GELU, preact=h, drop_p=0.1, seed=7)
        outs.append(h)
    if variant.startswith("gate"):
        assert ldc == n
        kw.update(epi_bwd=True, gate=t["gate"], act=L.ACT_GELU, drop_p=0.1, seed=9)
        if variant.endswith("colsum"):
            db = torch.zeros(n, device=dev)
            kw.update(db=db, db_ws=torch.zeros(((M + 63) // 64) * n, device=dev))
            outs.append(db)
    ops.gemm(A, B, C, **kw)
    torch.cuda.synchronize()
    return outs


@pytest.fixture(scope="module")
def inputs(dev):
    return {lay: _inputs(dev, lay) for lay in LAYOUTS}


@pytest.fixture(scope="module")
def generic(dev, inputs):
    """the generic epilogue's results (128x128 tile), computed once per (layout, variant, dtype)"""
    cache = {}

    def get(layout, variant, dtype):
        key = (layout, variant, dtype)
        if key not in cache:
            prev = L.set_option("gemm_tile", "128")
            try:
                cache[key] = _launch(dev, inputs[layout], variant, dtype)
            finally:
                L.set_option("gemm_tile", prev)
        return cache[key]
    return get


@pytest.mark.parametrize("tile", ["192", "192w8s3"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_variant_equals_generic_epilogue(dev, lib_opt, inputs, generic, layout, variant, tile):
    dtypes = [torch.bfloat16] if variant.endswith("colsum") else [torch.bfloat16, torch.float32]
    for dtype in dtypes:
        ref = generic(layout, variant, dtype)
        lib_opt("gemm_tile", tile)
        got = _launch(dev, inputs[layout], variant, dtype)
        lib_opt("gemm_tile", "auto")
        n_exact = len(got) - 1 if variant.endswith("colsum") else len(got)
        for i in range(n_exact):
            assert torch.equal(got[i], ref[i]), (layout, variant, tile, dtype, i, _rel(got[i], ref[i]))
        if variant.endswith("colsum"):
            assert _rel(got[-1], ref[-1]) < 1e-5


@pytest.mark.parametrize("tile", ["192", "192w8s3"])
@pytest.mark.parametrize("case", ["n_not_multiple_of_8", "unaligned_c", "batch2", "batch2_padded_c"])
def test_launches_outside_the_variants_conditions(dev, lib_opt, tile, case):
    """launches a variant must refuse (they run the generic epilogue) or must handle per batch:
    N % 8 != 0 (ragged last vector), a C that is not 16-byte aligned, batch offsets"""
    n, ldc, batch, c_off = N, None, 1, 0
    if case == "n_not_multiple_of_8":
        n, ldc = 1164, 1168
    elif case == "unaligned_c":
        c_off = 4
    elif case == "batch2":
        batch = 2
    else:
        batch, ldc = 2, N + 8       # a padded C: rows and batches stay 16-byte aligned
    inp = _inputs(dev, "fwd", n=n, batch=batch)
    for variant in ("bias", "bias_res_drop"):
        lib_opt("gemm_tile", "128")
        ref = _launch(dev, inp, variant, n=n, ldc=ldc, batch=batch, c_off=c_off)
        lib_opt("gemm_tile", tile)
        got = _launch(dev, inp, variant, n=n, ldc=ldc, batch=batch, c_off=c_off)
        assert torch.equal(got[0], ref[0]), (case, variant, tile)

"""CPU-side checks of the C-ABI boundary: the library loads and exports every entry
point declared in include/*.h, and the ctypes table matches the header (no GPU calls)."""
import ctypes
import glob
import os
import re

from avsr_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(avsr_[a-z0-9_]+)\s*\(", src))
    return names


def test_header_symbols_exported():
    lib = L.load()
    names = _declared()
    assert len(names) >= 5
    for n in sorted(names):
        assert hasattr(lib, n), f"{n} declared in include/ but not exported"


def test_ctypes_table_covers_header():
    assert _declared() <= set(L.SYMBOLS), sorted(_declared() - set(L.SYMBOLS))


def test_version_string():
    assert L.load().avsr_version().decode().startswith("avsr_hip")


def test_struct_sizes_match_c_layout():
    # int fields then 8-byte aligned pointers/int64: ctypes follows the C ABI
    assert ctypes.sizeof(L.GemmParams) % 8 == 0
    assert ctypes.sizeof(L.ConvParams) % 8 == 0


def test_conv_stat_tiles_per_dtype():
    """regression of the round-2 s3h fault: the BN partial-statistics buffer of a conv forward
    is sized by avsr_conv_stat_tiles, whose tile height must be the one the dtype's path
    launches — 192-row tiles on the bf16 LDS-DMA path where they pay (ResNet stage 2 at C2,
    M = 6000 x 11 x 11), the 128-row register-staged tile for fp32. Host-side query, no GPU."""
    from avsr_amd import ops
    g = ops.ConvGeom(6000, 11, 11, 128, 128, 3, 3, (1, 1), (1, 1))
    M = 6000 * 11 * 11
    assert ops.conv_stat_tiles(g, L.AVSR_BF16) == -(-M // 192)
    assert ops.conv_stat_tiles(g, L.AVSR_F32) == -(-M // 128)
    # a shape below the 192 rule stays on 128 rows for both
    g2 = ops.ConvGeom(8, 11, 11, 128, 128, 3, 3, (1, 1), (1, 1))
    assert ops.conv_stat_tiles(g2, L.AVSR_BF16) == ops.conv_stat_tiles(g2, L.AVSR_F32) == -(-8 * 121 // 128)
    # N <= 64 (stage 1): 256-row tiles on both paths
    g3 = ops.ConvGeom(6000, 22, 22, 64, 64, 3, 3, (1, 1), (1, 1))
    assert ops.conv_stat_tiles(g3, L.AVSR_BF16) == ops.conv_stat_tiles(g3, L.AVSR_F32) == -(-6000 * 484 // 256)


_BIG = (64, 16, 4096, 4096)      # B*H*Lq*ceil(Lk/2) > 2^32 - 1: the dropout pair index needs 64 bits
ATTN_PATH_TABLE = [
    # (B, H, Lq, Lk), keywords of ops.attn_path, forward path, backward path; bf16 unless the keywords say otherwise
    ((2, 2, 41, 41), dict(causal=True), "resident", "resident"),
    ((3, 2, 41, 150), {}, "resident", "resident"),
    ((2, 3, 200, 130), {}, "sq", "enc"),
    ((1, 2, 127, 127), {}, "resident", "resident"),
    ((1, 2, 128, 128), {}, "sq", "enc"),
    ((1, 2, 128, 127), {}, "sq", "resident"),
    ((1, 2, 384, 384), {}, "sq", "enc"),
    ((1, 2, 385, 385), {}, "sq", "tiled"),
    ((1, 2, 41, 385), {}, "tiled", "tiled"),
    ((1, 2, 385, 41), {}, "sq", "tiled"),
    ((1, 2, 200, 200), dict(causal=True), "resident", "resident"),
    ((1, 1, 400, 400), dict(causal=True), "tiled", "tiled"),
    ((1, 2, 200, 200), dict(lddo=2 * 64 + 4), None, "resident"),
    (_BIG, {}, "tiled", "tiled"),
    ((1, 2, 200, 200), dict(sq=0), "resident", "enc"),
    ((1, 2, 520, 520), dict(sq=0), "tiled", "tiled"),
    ((2, 2, 41, 41), dict(dtype=L.AVSR_F32), "f32", "f32"),
    ((1, 2, 520, 520), dict(dtype=L.AVSR_F32), "f32", "f32"),
]


def test_attn_path_table():
    """avsr_attn_path: which kernel family a shape runs, forward and backward, at every threshold
    of the choice (128 and 384 rows, causal, the 32-bit dropout index, lddo alignment, the
    attn_sq_fwd option, fp32); and the codes of a rejected call. Host-side query, no GPU."""
    import pytest
    import torch
    from avsr_amd import ops
    assert _BIG[0] * _BIG[1] * _BIG[2] * ((_BIG[3] + 1) // 2) > 0xFFFFFFFF
    for shape, kw, fwd, bwd in ATTN_PATH_TABLE:
        kw = dict(kw)
        dtype = kw.pop("dtype", torch.bfloat16)
        prev = L.set_option("attn_sq_fwd", kw.pop("sq", 1))
        try:
            if fwd is not None:
                assert ops.attn_path(dtype, *shape, **kw) == fwd, (shape, kw, "fwd")
            assert ops.attn_path(dtype, *shape, backward=True, **kw) == bwd, (shape, kw, "bwd")
        finally:
            L.set_option("attn_sq_fwd", prev)
    assert L.get_option("attn_sq_fwd") == 1
    with pytest.raises(L.AvsrLibError, match="1003"):                       # AVSR_E_DTYPE
        ops.attn_path(7, 2, 2, 41, 41)
    with pytest.raises(L.AvsrLibError, match="1002"):                       # AVSR_E_ALIGN
        ops.attn_path(torch.bfloat16, 1, 2, 200, 200, ld=132)
    p = L.fill(L.AttnParams, dtype=L.AVSR_BF16, B=1, H=2, Lq=200, Lk=200, ldq=128, ldk=128, ldv=128, ldo=128)
    assert L.load().avsr_attn_path(ctypes.byref(p), 2) == 1004              # AVSR_E_ARG: no such pass
    assert L.load().avsr_attn_path(None, 0) == 1004


_S1 = (6, 22, 22, 64, 64, 3, 1, 1)          # ResNet stage 1
_S2D = (5, 22, 22, 64, 128, 3, 2, 1)        # stage 2's stride-2 entry
_S4 = (4, 3, 3, 512, 512, 3, 1, 1)          # stage 4
_STEM = (3, 88, 88, 8, 64, 7, 2, 3)         # the stem as a 2-D conv over 8 packed channels
_POS = (3, 37, 1, 16, 16, 128, 1, 0)        # the grouped pos-conv (its ConvGeom keywords below)
_POS_KW = dict(groups=16, pad=(64, 0), kw=1, hout=37, wout=1)
# the patch kernel's span rule (conv.hip patch_ok) for 64 channels, H = W: 255 + 2 (255 // W + 1) +
# 2 (W + 2) (255 // W^2 + 1) + 2 (W + 3) + 1 <= PATCH_ROWS = 384 gives 384 at W = 24 and 388 at W = 25
CONV_PATH_TABLE = [
    # geometry (nimg, h, w, cin, cout, k, stride, pad); keywords (dtype, options by name, geom = ConvGeom
    # keywords, the rest flags of ops.conv_path); then (family, figure) of the forward, the data-grad and the
    # weight-grad with a workspace (None: not asked). Figure: the row-tile height (of every parity class
    # for s2); for a weight-grad on the general kernels the split-K slabs (1: no workspace).
    (_S1, {}, ("patch", 256), ("patch", 256), ("wpatch", None)),
    (_S1, dict(bias=True), ("glds", 256), None, None),
    (_S1, dict(act=L.ACT_GELU), ("glds", 256), None, None),
    (_S1, dict(res=True), ("glds", 256), None, None),
    (_S1, dict(preact=True), ("glds", 256), None, None),
    (_S1, dict(conv_patch=0), ("glds", 256), ("glds", 256), None),
    (_S1, dict(conv_wpatch=0), None, None, ("glds", 3)),
    (_S1, dict(ws=False), None, None, ("glds", None)),
    ((2, 24, 24, 64, 64, 3, 1, 1), {}, ("patch", 256), ("patch", 256), ("glds", 2)),
    ((2, 25, 25, 64, 64, 3, 1, 1), {}, ("glds", 256), ("glds", 256), ("glds", 2)),
    ((6, 11, 11, 64, 64, 3, 1, 1), {}, ("glds", 256), ("glds", 256), ("glds", 1)),      # span 409
    (_S2D, {}, ("glds", 128), ("s2", 256), ("glds", 1)),
    (_S2D, dict(conv_s2phase=0), None, ("glds", 256), None),
    ((2, 8, 8, 16, 32, 3, 2, 1), {}, ("glds", 256), ("glds", 256), ("glds", 1)),        # cout % 64 != 0
    ((6000, 11, 11, 128, 128, 3, 1, 1), {}, ("glds", 192), ("glds", 192), ("wpatch", None)),
    ((6000, 11, 11, 128, 128, 3, 1, 1), dict(conv_192=0), ("glds", 128), ("glds", 128), None),
    (_S4, {}, ("glds", 64), ("glds", 64), ("wpatch", None)),
    (_S4, dict(splitk=3), None, None, ("glds", 1)),
    (_S4, dict(ws=False), None, None, ("glds", None)),
    (_STEM, {}, ("glds", 256), ("s2", 256), ("stem_wpatch", None)),
    (_STEM, dict(stem_wpatch=0), None, None, ("glds", 6)),
    (_STEM, dict(ws=False), None, None, ("glds", None)),
    (_POS, dict(geom=_POS_KW), ("glds", 256), ("glds", 256), ("glds", 1)),
    (_S1, dict(dtype=L.AVSR_F32), ("reg", 256), ("reg", 256), ("reg", 3)),
    (_S2D, dict(dtype=L.AVSR_F32), ("reg", 128), ("reg", 256), ("reg", 1)),
    (_S4, dict(dtype=L.AVSR_F32), ("reg", 64), ("reg", 64), ("reg", 1)),
]


def _conv_geom(case, **kw):
    from avsr_amd import ops
    n, h, w, cin, cout, k, s, p = case
    return ops.ConvGeom(n, h, w, cin, cout, k, kw.pop("kw", k), kw.pop("stride", (s, s)), kw.pop("pad", (p, p)), **kw)


def test_conv_path_table():
    """avsr_conv_path: which kernel family a convolution runs per pass, on both sides of every
    threshold of the choice (the forward epilogue flags, each conv_* option, the PATCH_ROWS span,
    cout % 64 of the parity classes, the 192-row rule, a workspace and splitk for the weight-grad,
    fp32), and the codes of a rejected call. The three size queries a caller allocates by must give
    what the family and its tile imply: 256-row tiles for patch, the sum over the parity classes,
    128 x 64 x 576 floats for wpatch, 256 x 64 x 392 for stem_wpatch, the slabs of a general
    weight-grad. Host-side queries, no GPU."""
    import pytest
    from avsr_amd import ops
    lib = L.load()
    for case, kw, *passes in CONV_PATH_TABLE:
        kw = dict(kw)
        dtype = kw.pop("dtype", L.AVSR_BF16)
        g = _conv_geom(case, **kw.pop("geom", {}))
        opts = {k: kw.pop(k) for k in list(kw) if k in L.OPTIONS}
        prev = {k: L.set_option(k, v) for k, v in opts.items()}
        try:
            for pass_, want in zip(L.CONV_PASSES, passes):
                if want is None:
                    continue
                family, fig = want
                flags = dict(kw)
                if pass_ == "wgrad":
                    flags.setdefault("ws", True)
                assert ops.conv_path(g, dtype, pass_, **flags) == family, (case, kw, opts, pass_)
                p = g.params(dtype)
                p.splitk = flags.get("splitk", 0)
                if pass_ == "wgrad":
                    ktot = g.kh * g.kw * g.cin
                    ws = {"wpatch": 128 * 64 * 576, "stem_wpatch": 256 * 64 * 392}.get(family)
                    if ws is None and fig is not None:
                        ws = g.groups * fig * g.cout * ktot if fig > 1 else 0
                    if ws is not None:
                        assert lib.avsr_conv_wgrad_ws(ctypes.byref(p)) == ws, (case, kw, opts)
                elif family == "s2":
                    cls = [g.nimg * ((g.hin - a + 1) // 2) * ((g.win - b + 1) // 2) for a in (0, 1) for b in (0, 1)]
                    assert lib.avsr_conv_bnr_tiles(ctypes.byref(p)) == sum(-(-m // fig) for m in cls), (case, kw, opts)
                elif pass_ == "fwd":
                    assert lib.avsr_conv_stat_tiles(ctypes.byref(p)) == -(-g.out_pixels // fig), (case, kw, opts)
                else:
                    assert lib.avsr_conv_bnr_tiles(ctypes.byref(p)) == -(-g.in_pixels // fig), (case, kw, opts)
        finally:
            for k, v in prev.items():
                L.set_option(k, v)
    assert all(L.get_option(k) == 1 for k in ("conv_192", "conv_s2phase", "conv_patch", "conv_wpatch", "stem_wpatch"))
    for pass_ in L.CONV_PASSES:
        with pytest.raises(L.AvsrLibError, match="1001"):                   # AVSR_E_SHAPE: cin no power of two
            ops.conv_path(_conv_geom((6, 22, 22, 48, 64, 3, 1, 1)), L.AVSR_BF16, pass_)
        with pytest.raises(L.AvsrLibError, match="1002"):                   # AVSR_E_ALIGN: ldx % 8
            ops.conv_path(_conv_geom(_S1, ldx=68), L.AVSR_BF16, pass_)
        with pytest.raises(L.AvsrLibError, match="1003"):                   # AVSR_E_DTYPE
            ops.conv_path(_conv_geom(_S1), 7, pass_)
    p = _conv_geom(_S1).params(L.AVSR_BF16)
    assert lib.avsr_conv_path(ctypes.byref(p), 3) == 1004                    # AVSR_E_ARG: no such pass
    assert lib.avsr_conv_path(ctypes.byref(p), -1) == 1004
    assert lib.avsr_conv_path(None, 0) == 1004


def _zero_size_calls(dt):
    """(entry point, arguments) for the LayerNorm, BatchNorm, pooling, elementwise, packing and
    weight-norm entry points that take a dtype code: every call describes zero rows / images /
    elements with valid channel counts and strides, and holds no pointer"""
    ref = ctypes.byref
    ln = L.fill(L.LayerNormParams, dtype=dt, rows=0, N=64, ldx=64, ldy=64, lddy=64, lddx=64)
    bn = L.fill(L.BnActParams, dtype=dt, M=0, C=64)
    sp = L.fill(L.StemPoolParams, dtype=dt, nimg=0, H=4, W=4, C=64, Ho=2, Wo=2)
    ew = L.fill(L.EwParams, dtype=dt, rows=0, N=64, lddy=64, ldout=64, alpha=1.0)
    em = L.fill(L.EmbedParams, dtype=dt, rows=0, L=1, D=64)
    return [
        ("avsr_layernorm_fwd", (ref(ln), None)),
        ("avsr_layernorm_bwd", (ref(ln), None)),
        ("avsr_bn_act_fwd", (ref(bn), None)),
        ("avsr_bn_act_bwd_reduce", (ref(bn), None)),
        ("avsr_bn_bwd_apply", (ref(bn), None)),
        ("avsr_stem_pool_fwd", (ref(sp), None)),
        ("avsr_stem_pool_bwd_apply", (ref(sp), None)),
        ("avsr_avgpool_fwd", (dt, 0, 1, 64, None, None, None)),
        ("avsr_avgpool_bwd", (dt, 0, 1, 64, None, None, None)),
        ("avsr_ew_bwd", (ref(ew), None)),
        ("avsr_dropout_fwd", (ref(ew), None)),
        ("avsr_mask_rows", (dt, 0, 1, 64, None, 64, None, None)),
        ("avsr_embed_fwd", (ref(em), None)),
        ("avsr_embed_bwd", (ref(em), None)),
        ("avsr_stem_pack", (dt, 0, 0, None, None, None)),
        ("avsr_audio_pack", (dt, 0, 1, 1, None, None, None)),
        ("avsr_weightnorm_fwd", (dt, 0, 0, 0, None, None, None, None, None)),
    ]


def test_dtype_checked_first():
    """An unknown dtype code is AVSR_E_DTYPE (1003) before anything else an entry point does: the
    zero-size early return, the argument checks that need a pointer, any launch. The calls are
    over nothing and hold no pointers, so an entry point that got the order wrong returns 0 or
    another code, or launches over nothing; it never reads through a bad pointer. Only the null
    check of the params struct itself precedes the dtype (it has to). avsr_stem_wpack is not in
    the table: its size is fixed, so it cannot be called over nothing without pointers; with
    device buffers it is in test_gpu_loss_misc.py::test_stem_wpack_rejects_unknown_dtype.
    No GPU."""
    lib = L.load()
    for name, args in _zero_size_calls(7):
        assert getattr(lib, name)(*args) == 1003, name
    for name in ("avsr_layernorm_fwd", "avsr_bn_act_fwd", "avsr_stem_pool_fwd", "avsr_ew_bwd", "avsr_embed_fwd"):
        assert getattr(lib, name)(None, None) == 1004, name                 # AVSR_E_ARG: no params


def _header_option_defaults():
    """{AVSR_OPT_name: default} from the bracketed defaults in avsr_hip.h's option table"""
    src = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s+(AVSR_OPT_[A-Z0-9_]+)\s+\[(-?\d+)\]", src)}


def test_kernel_options_declared_and_defaulted():
    """every kernel-selection knob is a declared option (avsr_set_option / avsr_get_option) with
    the default the header documents; Python's name table covers them all"""
    lib = L.load()
    doc = _header_option_defaults()
    src = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(AVSR_OPT_[A-Z0-9_]+)\s*=\s*(\d+)", src)}
    count = ids.pop("AVSR_OPT_COUNT")
    assert set(doc) == set(ids) and len(ids) == count == len(L.OPTIONS)
    for name, i in ids.items():
        assert lib.avsr_get_option(i) == doc[name], name
        assert L.OPTIONS[name[len("AVSR_OPT_"):].lower()] == i
    assert lib.avsr_get_option(count) == -1 and lib.avsr_get_option(-1) == -1


def test_tile_names_match_header():
    """the AVSR_TILE_* ids of avsr_hip.h are dense, and their names in id order are Python's
    TILES (set_option turns a tile name into its id by position)"""
    src = open(os.path.join(ROOT, "include", "avsr_hip.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bAVSR_TILE_([A-Za-z0-9]+)\s*=\s*(\d+)", src)}
    count = ids.pop("COUNT")
    assert sorted(ids.values()) == list(range(count))
    assert [n.lower() for n in sorted(ids, key=ids.get)] == L.TILES
    assert count == len(L.TILES)


def test_set_option_roundtrip_and_range():
    lib = L.load()
    assert lib.avsr_set_option(L.OPTIONS["attn_sq_bwd"], 2) == 1004          # AVSR_E_ARG: out of range
    assert lib.avsr_set_option(99, 0) == 1004                                  # unknown option
    prev = L.set_option("gemm_tile", "192")
    try:
        assert L.get_option("gemm_tile") == L.TILES.index("192") + 1
        assert lib.avsr_set_option(L.OPTIONS["gemm_tile"], len(L.TILES) + 1) == 1004
    finally:
        L.set_option("gemm_tile", prev)
    assert L.get_option("gemm_tile") == 0


def test_library_reads_no_environment():
    """kernel selection does not depend on process environment: no getenv in the sources, and
    the built library imports no getenv"""
    for f in glob.glob(os.path.join(ROOT, "avsr_amd", "csrc", "*")):
        assert "getenv" not in open(f).read(), f
    import subprocess
    out = subprocess.run(["nm", "-D", "--undefined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in out

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

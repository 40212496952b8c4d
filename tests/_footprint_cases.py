"""The forward case table of the guard-zone tests: imported by tests/test_sizes_cpu.py (which asserts, with the library's host-side
route logic and no GPU, that the table reaches every GEMM route / tile height for at least two dtypes) and by
tests/test_gpu_footprint.py (which runs every row through the C ABI between guard zones)."""
from __future__ import annotations

from collections import namedtuple

import torch

from benchlib.workloads import A16_Q, INT_Q, INTROW_Q, MXINT_Q, W8A8_Q, _bfp

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _mf(w, ew, eb):
    return dict(name="minifloat", width=w, exponent_width=ew, exponent_bias=eb)


CONFIGS = {
    "mx": MXINT_Q,                                                             # W4A8 MXINT, blocks of 16 everywhere
    "mx_pass": dict(MXINT_Q, B_out_quantizer=dict(name="passthrough")),        # B_out pass-through
    "mx_row": dict(MXINT_Q, B_out_quantizer=_bfp(8, [1, -1], True)),           # B_out one block per row: the pre-pass
    "mx_b64": dict(MXINT_Q, B_out_quantizer=_bfp(8, [1, 64], True)),           # B_out blocks of 64: the pre-pass, several blocks per row
    "mx_w8": dict(MXINT_Q, w_quantizer=_bfp(8, [1, 16], False)),               # 8-bit weights in blocks of 16: three 4-bit limb images
    "int": INT_Q,                                                              # per-token x, W blocks of 128, A / B unquantized: int8 route
    "introw": INTROW_Q,                                                        # ... one weight block per row
    "w8a8": W8A8_Q,                                                            # 8-bit weights, one block per row: the int8 image of codes
    "a16": A16_Q,                                                              # pass-through activations
    "intw": dict(MXINT_Q, w_quantizer=dict(name="integer", width=4, frac_width=7)),   # integer weights (two's-complement nibbles)
    "mfw": dict(MXINT_Q, w_quantizer=_mf(4, 2, 7)),                            # minifloat weights (e4m3 table)
}
UNQUANTIZED_AB = ("int", "introw", "w8a8", "a16")

# x_kind: what the module's packing must decide for the descriptor's x format ("mx" block_fp, "i8" LQER_Q_MXINT_I8, "f16"
# LQER_Q_PASSTHROUGH_F16, "pass" pass-through limbs) - the GPU test asserts it, so that the routes computed on the CPU are the ones run.
# route / rows: what lqer_gemm_route / lqer_gemm_tile_rows must say.  tune: names of _lib.TUNE_* bits.  flags: module attributes.
Case = namedtuple("Case", "id cfg K N r M dtype bias tune ldy_pad ldx_pad x_kind route rows flags")


def _c(id, cfg, K, N, r, M, dtype, x_kind, route, rows, bias=False, tune=(), ldy_pad=0, ldx_pad=0, **flags):
    return Case(id, cfg, K, N, r, M, dtype, bias, tuple(tune), ldy_pad, ldx_pad, x_kind, route, rows, dict(flags))


S, T128, T256, I8 = "SMALLM", "TILE128", "TILE256", "I8"

CASES = [
    # ---- block-16 MXINT: decode kernels (one launch up to 8 tokens with 16-byte rows, two launches otherwise)
    _c("mx-decode1-m1", "mx", 128, 48, 16, 1, "f16", "mx", S, 0),
    _c("mx-decode1-m5-pad8", "mx", 128, 48, 16, 5, "bf16", "mx", S, 0, bias=True, ldy_pad=8, ldx_pad=8),
    _c("mx-decode1-m8-ldy3", "mx", 208, 1000, 20, 8, "f32", "mx", S, 0, ldy_pad=3),
    _c("mx-decode2-m7-ldx5", "mx", 128, 48, 16, 7, "f16", "mx", S, 0, ldy_pad=3, ldx_pad=5),       # rows not 16-byte aligned
    _c("mx-decode2-m33", "mx", 200, 1000, 32, 33, "f32", "mx", S, 0, bias=True, ldy_pad=3, ldx_pad=5),
    _c("mx-decode2-m63", "mx_pass", 128, 1000, 16, 63, "bf16", "mx", S, 0, ldy_pad=8, ldx_pad=8),
    _c("mx-smallm-m64-rank0", "mx", 128, 48, 0, 64, "f16", "mx", S, 0, ldy_pad=3),
    # ---- 128-row kernel family on 64-row tiles
    _c("mx-t64-m65", "mx", 128, 48, 16, 65, "f16", "mx", T128, 64, ldy_pad=8),
    _c("mx-t64-m127-ldy3", "mx", 200, 1000, 20, 127, "bf16", "mx", T128, 64, bias=True, ldy_pad=3, ldx_pad=8),
    _c("mx-t64-m300", "mx_pass", 128, 1000, 32, 300, "f32", "mx", T128, 64, ldy_pad=3, ldx_pad=5),
    _c("mx-t64-m129-row", "mx_row", 128, 1000, 16, 129, "f16", "mx", T128, 64, ldy_pad=8),
    _c("mx-t64-m65-b64", "mx_b64", 128, 1000, 16, 65, "bf16", "mx", T128, 64, ldy_pad=3),
    # ---- ... on 128-row tiles (pinned at small shapes; natural at 4097 x 4096)
    _c("mx-t128-m129", "mx", 128, 1000, 16, 129, "f16", "mx", T128, 128, tune=("TILE_ROWS_128",), ldy_pad=8),
    _c("mx-t128-m127-ldy3", "mx", 200, 48, 20, 127, "bf16", "mx", T128, 128, bias=True, tune=("TILE_ROWS_128",), ldy_pad=3, ldx_pad=5),
    _c("mx-t128-m300-f32", "mx_row", 128, 1000, 32, 300, "f32", "mx", T128, 128, tune=("TILE_ROWS_128",), ldy_pad=3, ldx_pad=8),
    _c("mx-t128-m4097", "mx", 128, 4096, 16, 4097, "f16", "mx", T128, 128),
    _c("mx-t128-defer-k1024", "mx", 1024, 48, 16, 130, "bf16", "mx", T128, 128, tune=("TILE_ROWS_128",), ldy_pad=3),
    _c("mx-t128-prologue-k1024", "mx", 1024, 48, 16, 130, "bf16", "mx", T128, 128, tune=("TILE_ROWS_128", "BOUT_IN_PROLOGUE"), ldy_pad=3),
    _c("mx-t128-defer-k1024-f16", "mx", 1024, 1000, 32, 257, "f16", "mx", T128, 128, tune=("TILE_ROWS_128",), ldy_pad=8, ldx_pad=8),
    # ---- block-16 activations through the image with the fragment-major copy (a_limbs = -2)
    _c("mx-act16-fused-m300", "mx", 128, 1000, 16, 300, "f16", "mx", T128, 64, tune=("ACT16_FUSED",), ldy_pad=8, ldx_pad=8),
    _c("mx-act16-fused-m1025", "mx", 256, 48, 32, 1025, "bf16", "mx", T128, 64, ldy_pad=3),
    _c("mx-act16-split-m1100", "mx", 128, 1000, 64, 1100, "f16", "mx", T128, 64, tune=("ACT16_SPLIT",), ldy_pad=3),
    # ---- 256-row tiles
    _c("mx-t256-m2817", "mx", 128, 4096, 16, 2817, "f16", "mx", T256, 256, ldy_pad=8),
    _c("mx-t256-m2815-ldy3", "mx_pass", 128, 4096, 16, 2815, "bf16", "mx", T256, 256, bias=True, ldy_pad=3, ldx_pad=8),
    # ---- integer / minifloat / 8-bit limb weights (the 128-row tile kernel at every token count; limbs: every route)
    _c("intw-m1", "intw", 128, 48, 16, 1, "f16", "mx", T128, 128, ldy_pad=3),
    _c("intw-m70", "intw", 200, 1000, 16, 70, "bf16", "mx", T128, 128, ldy_pad=8, ldx_pad=5),
    _c("mfw-m129", "mfw", 128, 1000, 16, 129, "f16", "mx", T128, 128, ldy_pad=3),
    _c("mfw-m3", "mfw", 128, 48, 16, 3, "f32", "mx", T128, 128, bias=True, ldy_pad=3),
    _c("w8limbs-m5", "mx_w8", 128, 48, 16, 5, "f16", "mx", S, 0, ldy_pad=3),
    _c("w8limbs-m200", "mx_w8", 200, 1000, 16, 200, "bf16", "mx", T128, 64, ldy_pad=3, ldx_pad=8),
    _c("w8a8-limbs-m300", "w8a8", 128, 1000, 32, 300, "f16", "mx", T128, 64, ldy_pad=8, a8_native=False),
    # ---- int8 route: 128- and 256-row tiles, the pre-pass variants of the B_out row maxima, the one-launch activation side
    _c("int-i8-128-xch", "int", 128, 1000, 32, 300, "f16", "i8", I8, 128, ldy_pad=8),
    _c("int-i8-128-xch-miss", "int", 128, 1000, 32, 300, "f16", "i8", I8, 128, tune=("AMAX_XCH_MISS",), ldy_pad=3),
    _c("int-i8-128-atomic", "int", 128, 1000, 32, 257, "bf16", "i8", I8, 128, tune=("AMAX_ATOMIC",), ldy_pad=3, ldx_pad=8),
    _c("int-i8-128-parts", "introw", 200, 1000, 16, 255, "f16", "i8", I8, 128, tune=("AMAX_PARTS",), ldy_pad=8, ldx_pad=5),
    _c("int-i8-128-f32", "int", 128, 48, 64, 129, "f32", "i8", I8, 128, bias=True, ldy_pad=3),
    _c("int-i8-256-pinned", "int", 128, 1000, 32, 300, "bf16", "i8", I8, 256, tune=("I8_ROWS_256",), ldy_pad=3),
    _c("int-i8-256-m3000", "int", 128, 4096, 32, 3000, "f16", "i8", I8, 256, ldy_pad=8),
    _c("int-i8-mrx-m2047", "int", 128, 4352, 32, 2047, "f16", "i8", I8, 128, tune=("I8_ROWS_128",)),           # several rounds, in-GEMM items
    _c("int-i8-no-mrx-m2047", "int", 128, 4352, 32, 2047, "f16", "i8", I8, 128, tune=("I8_ROWS_128", "AMAX_NO_MRX")),
    _c("int-act8-fused-m300", "int", 128, 1000, 32, 300, "f16", "i8", I8, 128, tune=("ACT8_FUSED",), ldy_pad=3, ldx_pad=8),
    _c("int-act8-fused-m1025", "introw", 256, 48, 16, 1025, "bf16", "i8", I8, 128, ldy_pad=8),
    _c("int-act8-split-m1100", "int", 128, 1000, 32, 1100, "f16", "i8", I8, 128, tune=("ACT8_SPLIT",), ldy_pad=3),
    _c("int-limbs-a-m300", "int", 128, 1000, 32, 300, "f16", "i8", I8, 128, ldy_pad=3, i8_a_f16=False),       # A as bf16 limbs
    _c("int-below-i8-m65", "int", 128, 1000, 32, 65, "f16", "i8", T128, 64, ldy_pad=3),                       # bf16 kernels on the same buffers
    _c("int-below-i8-m1", "int", 128, 48, 32, 1, "bf16", "i8", T128, 128, ldy_pad=3),
    _c("w8a8-i8-128", "w8a8", 128, 1000, 32, 300, "f16", "i8", I8, 128, ldy_pad=3),
    _c("w8a8-i8-256", "w8a8", 256, 1000, 32, 257, "bf16", "i8", I8, 256, tune=("I8_ROWS_256",), ldy_pad=8, ldx_pad=8),
    # ---- pass-through activations: the fp16 route (incl. the tensor as its own image: xq == x) and bf16 limbs
    _c("a16-f16-m256-dense", "a16", 128, 1000, 32, 256, "f16", "f16", T128, 64, ldy_pad=8),
    _c("a16-f16-m64-dense", "a16", 128, 48, 32, 64, "f16", "f16", S, 0, ldy_pad=3),
    _c("a16-f16-m300-ldx8", "a16", 200, 1000, 32, 300, "f16", "f16", T128, 64, ldy_pad=3, ldx_pad=8),
    _c("a16-limbs11-m65", "a16", 128, 1000, 32, 65, "f16", "pass", T128, 64, ldy_pad=3, ldx_pad=5, a16_native=False),
    _c("a16-limbs8-m129", "a16", 128, 48, 16, 129, "bf16", "pass", T128, 64, ldy_pad=8),
    _c("a16-limbs24-m1", "a16", 128, 48, 16, 1, "f32", "pass", S, 0, ldy_pad=3),
    _c("a16-limbs24-m130", "a16", 200, 1000, 16, 130, "f32", "pass", T128, 128, bias=True, tune=("TILE_ROWS_128",), ldy_pad=3, ldx_pad=5),
]

# every (route, tile rows) pair the table must reach for at least two dtypes each (tests/test_sizes_cpu.py)
REQUIRED_ROUTES = [(S, 0), (T128, 64), (T128, 128), (T256, 256), (I8, 128), (I8, 256)]


def tuning_bits(case) -> int:
    from lqer_amd import _lib

    bits = 0
    for name in case.tune:
        bits |= getattr(_lib, "TUNE_" + name)
    return bits


def make_module(case, device=None):
    """The module of a case, unpacked (its descriptor's x format is then decided by hand on the CPU, by the packing on the GPU)."""
    import lqer_amd

    qc = CONFIGS[case.cfg]
    if case.r > 0:
        mod = lqer_amd.LinearFlexibleLqer(case.K, case.N, bias=case.bias, q_config=qc, l_config={"rank": case.r})
    else:
        mod = lqer_amd.LinearFlexible(case.K, case.N, bias=case.bias, q_config=dict(qc, name="flexible"))
    for k, v in case.flags.items():
        assert hasattr(mod, k), k
        setattr(mod, k, v)
    mod.tuning = tuning_bits(case)
    return mod


def host_desc(case):
    """The descriptor the GPU run will use, built without a GPU: the x format the packing is expected to choose is set by hand."""
    mod = make_module(case).to(DTYPES[case.dtype])
    mod._x_i8 = case.x_kind == "i8"
    mod._x_f16 = case.x_kind == "f16"
    return mod._desc()

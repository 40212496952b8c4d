"""Operands and cases of tests/test_gpu_exact_routes.py (checked without a GPU by tests/test_exact_cases_cpu.py): the WHOLE Linear forward
- main product, side path, bias - on operands whose fp32 partial sums are exact in any order, so that the oracle determines every bit of
y on every GEMM route.  tests/_gemm256_cases.py does this for the main product of one geometry; here it is one builder for any shape and
quantizer configuration, and a case table over the routes.

Operands of a fixture (numpy PCG64, seeded by the fixture's id; every value exact in fp32, fp16 and bf16 alike):
  x     N(0, 1) rounded to 8 significant bits, channel 7 times 16, a zero row, a zero block, a zero block in the last row;
        pass-through fp16 activations (A16_Q): multiples of 2^-5 instead, so that the grid unit does not follow the smallest element
  W     0.02 N(0, 1) times a power of two per (row, weight block) over SPREAD = 5 binades, 8 significant bits; a zero block, and row
        N - 1 - the last live column - zero
  A, B  integers -7 .. 7 times 2^-9: on the 8-bit MXINT grid, one bf16 limb, exact in fp16
  bias  multiples of 2^-12
Then every stage of O.lqer_linear_forward(..., intermediates=True) - xA, xAB, y - is a sum of multiples of a grid unit u (the lowest
set bit over the non-zero values that take part) whose magnitudes add up to less than 2^24 u: exact in fp32 in any order, under any
split of k, limb split or expand.  The three bounds (sum of magnitudes over 2^24 u) are computed per fixture and asserted < 1 by both
test files before anything is compared.  The coarse grids also put exact rounding ties in front of the A_out and B_out re-quantizers.

Measured on the CPU, per fixture of the table below (id = configuration, M, K, N, rank): the three bounds as fractions of 2^24 grid
units, and the elements that meet an exact rounding tie in front of the A_out / B_out re-quantizer (pass-through B_out: none):
  fixture                                x A  (xA)q B       y   ties A_out / B_out (of elements)
  mx-m8-k320-n272-r32                 0.0048   0.0015  0.0933   3 / 70  (256 / 2176)
  mx-m1-k320-n272-r32                 0.0036   0.0003  0.0711   0 / 14  (32 / 272)
  mx-m8-k1088-n272-r32                0.0137   0.0008  0.1176   1 / 68  (256 / 2176)
  mx-m8-k1088-n264-r16                0.0287   0.0005  0.5304   0 / 109  (128 / 2112)
  mx-m1-k1088-n260-r48                0.0246   0.0009  0.4329   0 / 6  (48 / 260)
  mx-m8-k320-n260-r48                 0.0044   0.0017  0.0542   1 / 53  (384 / 2080)
  mx_pass-m8-k1088-n272-r32           0.0134   0.0007  0.2329   0 / 0  (256 / 2176)
  mx_pass-m1-k320-n264-r16            0.0036   0.0002  0.0665   0 / 0  (16 / 264)
  opt-m8-k320-n272-r32-bias           0.0050   0.0017  0.0650   3 / 61  (256 / 2176)
  opt-m1-k1088-n264-r16-bias          0.0258   0.0001  0.2229   0 / 21  (16 / 264)
  mx-m8-k320-n272-r0                       -        -  0.0530   -
  mx-m1-k1088-n260-r0                      -        -  0.1115   -
  w2b32-m8-k320-n272-r32              0.0046   0.0012  0.0143   0 / 88  (256 / 2176)
  w2b32-m20-k320-n272-r32             0.0046   0.0014  0.0116   4 / 182  (640 / 5440)
  w3b16-m8-k320-n272-r32              0.0043   0.0005  0.0219   3 / 77  (256 / 2176)
  w3b16-m20-k320-n272-r32             0.0095   0.0011  0.0999   5 / 183  (640 / 5440)
  mx-m9-k320-n272-r32                 0.0047   0.0010  0.0439   1 / 76  (288 / 2448)
  mx-m16-k1088-n264-r32               0.0284   0.0009  0.2398   2 / 172  (512 / 4224)
  mx-m17-k320-n260-r0                      -        -  0.0508   -
  mx-m33-k1088-n272-r32               0.0272   0.0009  0.2617   5 / 386  (1056 / 8976)
  mx-m33-k320-n272-r0                      -        -  0.1112   -
  mx_pass-m48-k320-n264-r32           0.0097   0.0015  0.2425   9 / 0  (1536 / 12672)
  mx-m49-k1088-n260-r32               0.0281   0.0012  0.5228   5 / 514  (1568 / 12740)
  mx-m64-k320-n272-r32                0.0099   0.0016  0.1101   15 / 719  (2048 / 17408)
  mx-m64-k1088-n272-r0                     -        -  0.2559   -
  mx_pass-m64-k1088-n260-r32          0.0283   0.0009  0.5284   11 / 0  (2048 / 16640)
  mx-m130-k320-n272-r32               0.0096   0.0019  0.1299   23 / 1402  (4160 / 35360)
  mx-m65-k1024-n264-r32               0.0268   0.0009  0.2427   7 / 716  (2080 / 17160)
  mx-m65-k320-n260-r0                      -        -  0.1122   -
  mx-m130-k1024-n272-r0                    -        -  0.5161   -
  opt-m130-k1024-n272-r32-bias        0.0269   0.0021  0.2630   19 / 1471  (4160 / 35360)
  mx_pass-m130-k320-n260-r32          0.0099   0.0020  0.2255   35 / 0  (4160 / 33800)
  mx-m128-k320-n264-r0                     -        -  0.1220   -
  mx-m130-k320-n260-r48               0.0096   0.0022  0.2338   42 / 1041  (6240 / 33800)
  mx-m130-k1024-n272-r32              0.0265   0.0009  0.2406   13 / 1417  (4160 / 35360)
  mx-m130-k1088-n272-r32              0.0285   0.0009  0.4974   15 / 1492  (4160 / 35360)
  mx-m128-k1024-n260-r8               0.0279   0.0008  0.2797   4 / 2702  (1024 / 33280)
  mx-m130-k1024-n272-r48              0.0270   0.0016  0.5166   24 / 1003  (6240 / 35360)
  mx_pass-m130-k1024-n272-r32         0.0267   0.0010  0.2509   18 / 0  (4160 / 35360)
  mx_row-m130-k320-n272-r32           0.0102   0.0018  0.1351   33 / 865  (4160 / 35360)
  mx_row-m128-k1024-n264-r32          0.0267   0.0010  0.5216   13 / 808  (4096 / 33792)
  mx_row-m7-k320-n272-r32             0.0045   0.0010  0.0610   2 / 38  (224 / 1904)
  int-m130-k384-n272-r32              0.0029   0.0017  0.0235   207 / 1241  (4160 / 35360)
  int-m130-k1024-n272-r0                   -        -  0.0411   -
  int-m258-k1024-n272-r64             0.0067   0.0020  0.0415   496 / 1815  (16512 / 70176)
  introw-m130-k1024-n264-r32          0.0068   0.0009  0.0582   136 / 1288  (4160 / 34320)
  w8a8-m130-k384-n272-r32             0.0029   0.0015  0.4357   250 / 1178  (4160 / 35360)
  int-m258-k384-n264-r0                    -        -  0.0220   -
  introw-m258-k384-n260-r32           0.0028   0.0009  0.0264   428 / 2211  (8256 / 67080)
  w8a8-m258-k1024-n272-r64            0.0068   0.0017  0.9791   564 / 1801  (16512 / 70176)
  w8a8-m258-k384-n272-r0                   -        -  0.5142   -
  a16-m8-k320-n272-r0                      -        -  0.0378   -
  a16-m130-k320-n272-r0                    -        -  0.0241   -
  mx-m4098-k320-n2276-r32-bias        0.0111   0.0059  0.3625   1008 / 365551  (131136 / 9327048)
  mx-m3-k320-n272-r32                 0.0044   0.0006  0.0439   2 / 26  (96 / 816)
  mx-m3-k320-n144-r32                 0.0045   0.0004  0.0892   0 / 17  (96 / 432)
  opt-m3-k320-n272-r32-bias           0.0044   0.0008  0.0479   3 / 29  (96 / 816)
The largest: x A 0.0287, (xA)q B 0.0059, y 0.9791 (8-bit weights against 8-bit per-token activations over K = 1024; the int8 kernel
accumulates such products in integers).  Every side-path fixture of M >= 64 meets at least 4 ties in front of A_out and, where B_out
quantizes, 716 in front of it; the decode-size fixtures (M < 64) 49 and 2190 taken together.

The A16 side path is left out: its pass-through A_out carries x A as two bf16 limbs, and keeping x A within 16 bits needs a fixture of
its own.  A16_Q appears with rank 0 only (the fp16 main loop)."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from benchlib.workloads import A16_Q, INT_Q, INTROW_Q, MXINT_Q, OPT_Q, W8A8_Q, _bfp

DEV = "cuda:0"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
SPREAD = 5       # binades of the per-(row, block) power of two of W (tests/_gemm256_cases.py)
OUTLIER = 16.0   # factor of the outlier channel 7

CONFIGS = {
    "mx": MXINT_Q,                                                        # W4A8 MXINT, blocks of 16 everywhere
    "opt": OPT_Q,                                                         # ... bias in blocks of 16
    "mx_pass": dict(MXINT_Q, B_out_quantizer=dict(name="passthrough")),   # B_out pass-through
    "mx_row": dict(MXINT_Q, B_out_quantizer=_bfp(8, [1, -1], True)),      # B_out one block per row: the pre-pass
    "w2b32": dict(MXINT_Q, w_quantizer=_bfp(2, [1, 32], False)),          # 2- / 3-bit weights: the compact image
    "w3b16": dict(MXINT_Q, w_quantizer=_bfp(3, [1, 16], False)),
    "int": INT_Q,                                                         # per-token x, W blocks of 128: the int8 kernel
    "introw": INTROW_Q,                                                   # ... one weight block per row
    "w8a8": W8A8_Q,                                                       # ... 8-bit weights: the image of codes
    "a16": A16_Q,                                                         # pass-through fp16 activations (rank 0 here)
}

# a fixture: the operands and the oracle's stages of one (configuration, shape); xs: the id whose x it shares (a group's members)
Fx = namedtuple("Fx", "cfg M K N r bias xs")
# a case: a fixture run at one element type under tuning pins.  x_kind / route / rows / partials: what the packing and the plan must
# answer (asserted without a GPU and again before the run); kernel: the name of the piece the case is there for (printed); image:
# "narrow" = the compact weight image; flags: module attributes
Case = namedtuple("Case", "id fx dtype tune x_kind route rows partials kernel image flags")

S, T128, T256, I8 = "SMALLM", "TILE128", "TILE256", "I8"


def fx_id(fx) -> str:
    return f"{fx.cfg}-m{fx.M}-k{fx.K}-n{fx.N}-r{fx.r}" + ("-bias" if fx.bias else "")


def _case(kernel, cfg, M, K, N, r, dtype, route, rows, bias=False, tune=(), x_kind="mx", image="standard", xs=None, **flags):
    fx = Fx(cfg, M, K, N, r, bias, xs)
    partials = int(route == S and r > 0 and x_kind == "mx")  # lqer_decode_partials: the small-M kernel sums the partial tiles of x A itself
    cid = "-".join([kernel, fx_id(fx), dtype] + [t.lower() for t in tune])
    return Case(cid, fx, dtype, tuple(tune), x_kind, route, rows, partials, kernel, image, dict(flags))


def _table():
    c, out = _case, []
    # ---- one-launch decode (decode1.hip): M <= 8, K in whole blocks of 16; K = 1088: five slabs, the last one short.  N = 272: a last
    # column tile of 16; 264: a row stride that is an odd multiple of 8; 260: N % 8 != 0, the narrow 16-bit stores
    out += [c("decode1", "mx", 8, 320, 272, 32, dt, S, 0) for dt in ("f16", "bf16", "f32")]
    out += [c("decode1", "mx", 8, 320, 272, 32, "f16", S, 0, tune=("DECODE_NO_POLL",)),
            c("decode1", "mx", 1, 320, 272, 32, "f16", S, 0),
            c("decode1", "mx", 8, 1088, 272, 32, "f16", S, 0),
            c("decode1", "mx", 8, 1088, 264, 16, "bf16", S, 0),
            c("decode1", "mx", 1, 1088, 260, 48, "f32", S, 0),
            c("decode1", "mx", 8, 320, 260, 48, "f16", S, 0),
            c("decode1", "mx_pass", 8, 1088, 272, 32, "f16", S, 0),
            c("decode1", "mx_pass", 1, 320, 264, 16, "bf16", S, 0, tune=("DECODE_NO_POLL",)),
            c("decode1", "opt", 8, 320, 272, 32, "bf16", S, 0, bias=True),
            c("decode1", "opt", 1, 1088, 264, 16, "f16", S, 0, bias=True),
            # rank 0 at decode sizes: the small-M kernel alone, one token tile
            c("smallm-mt1", "mx", 8, 320, 272, 0, "f16", S, 0),
            c("smallm-mt1", "mx", 1, 1088, 260, 0, "f32", S, 0)]
    # ---- the compact 2- / 3-bit image read directly: one launch at M = 8, quantizer + small-M kernel at M = 20
    for cfg in ("w2b32", "w3b16"):
        out += [c("decode1-narrow", cfg, 8, 320, 272, 32, "f16", S, 0, image="narrow"),
                c("smallm-narrow-mt2", cfg, 20, 320, 272, 32, "bf16", S, 0, image="narrow")]
    # ---- small-M two-launch route (gemm_smallm.hip): every count of 16-row token tiles (mt = 1 .. 4) and their edges
    out += [c("smallm-mt1", "mx", 9, 320, 272, 32, "f16", S, 0),
            c("smallm-mt1", "mx", 16, 1088, 264, 32, "bf16", S, 0),
            c("smallm-mt2", "mx", 17, 320, 260, 0, "f32", S, 0),
            c("smallm-mt3", "mx", 33, 1088, 272, 32, "f16", S, 0),
            c("smallm-mt3", "mx", 33, 320, 272, 0, "f16", S, 0),
            c("smallm-mt3", "mx_pass", 48, 320, 264, 32, "bf16", S, 0),
            c("smallm-mt4", "mx", 49, 1088, 260, 32, "f32", S, 0),
            c("smallm-mt4", "mx", 64, 320, 272, 32, "f16", S, 0),
            c("smallm-mt4", "mx", 64, 1088, 272, 0, "bf16", S, 0),
            c("smallm-mt4", "mx_pass", 64, 1088, 260, 32, "f16", S, 0)]
    # ---- 64-row tiles: the plan's own choice at these shapes
    out += [c("tile64", "mx", 130, 320, 272, 32, dt, T128, 64) for dt in ("f16", "bf16", "f32")]
    out += [c("tile64", "mx", 65, 1024, 264, 32, "f16", T128, 64),
            c("tile64", "mx", 65, 320, 260, 0, "bf16", T128, 64),
            c("tile64", "mx", 130, 1024, 272, 0, "f32", T128, 64),
            c("tile64", "opt", 130, 1024, 272, 32, "bf16", T128, 64, bias=True),
            c("tile64", "mx_pass", 130, 320, 260, 32, "f16", T128, 64)]
    # ---- 128-row tiles (pinned).  K = 320: B_out re-quantized in front of the main loop; K >= 1024: under it (deferred), with the
    # k-split wave pairs unless the side product is staged through LDS (padded rank above LQER_STAGE_MIN = 32) or pinned off; every pin
    # must give the oracle's bits
    r128 = ("TILE_ROWS_128",)
    out += [c("tile128-prologue", "mx", 130, 320, 272, 32, "f16", T128, 128, tune=r128),
            c("tile128-prologue", "mx", 128, 320, 264, 0, "f16", T128, 128, tune=r128),
            c("tile128-prologue-staged", "mx", 130, 320, 260, 48, "bf16", T128, 128, tune=r128)]
    out += [c("tile128-defer-ksplit", "mx", 130, 1024, 272, 32, dt, T128, 128, tune=r128) for dt in ("f16", "bf16", "f32")]
    out += [c("tile128-defer", "mx", 130, 1024, 272, 32, "f16", T128, 128, tune=r128 + ("NO_KSPLIT",)),
            c("tile128-prologue", "mx", 130, 1024, 272, 32, "f16", T128, 128, tune=r128 + ("BOUT_IN_PROLOGUE",)),
            c("tile128-defer-ksplit-table", "mx", 130, 1024, 272, 32, "bf16", T128, 128, tune=r128 + ("W_EXP_TABLE",)),
            c("tile128-prologue-table", "mx", 130, 320, 272, 32, "f16", T128, 128, tune=r128 + ("W_EXP_TABLE",)),
            c("tile128-defer-ksplit", "mx", 130, 1088, 272, 32, "bf16", T128, 128, tune=r128),
            c("tile128-defer-ksplit", "mx", 128, 1024, 260, 8, "f32", T128, 128, tune=r128),       # rank 8, padded to 16
            c("tile128-defer-staged", "mx", 130, 1024, 272, 48, "f16", T128, 128, tune=r128),
            c("tile128-prologue-staged", "mx", 130, 1024, 272, 48, "bf16", T128, 128, tune=r128 + ("BOUT_IN_PROLOGUE",)),
            c("tile128-bout-pass", "mx_pass", 130, 1024, 272, 32, "f16", T128, 128, tune=r128),
            c("tile128-bout-row", "mx_row", 130, 320, 272, 32, "f16", T128, 128, tune=r128),        # the pre-pass of row maxima
            c("tile128-bout-row", "mx_row", 128, 1024, 264, 32, "bf16", T128, 128, tune=r128),
            c("tile128", "mx", 130, 1024, 272, 0, "bf16", T128, 128, tune=r128),
            # one block per row at a decode size: the small-M kernel has no pre-pass, the tile kernel takes the call
            c("tile128-bout-row-decode", "mx_row", 7, 320, 272, 32, "f16", T128, 128)]
    # ---- the int8 kernel, both tile heights pinned: weight blocks of 128, one per row, 8-bit codes; how the B_out row maxima travel
    i128, i256 = ("I8_ROWS_128",), ("I8_ROWS_256",)
    out += [c("i8-128", "int", 130, 384, 272, 32, "f16", I8, 128, tune=i128, x_kind="i8"),
            c("i8-128", "int", 130, 384, 272, 32, "f16", I8, 128, tune=i128 + ("AMAX_ATOMIC",), x_kind="i8"),
            c("i8-128", "int", 130, 384, 272, 32, "f16", I8, 128, tune=i128 + ("AMAX_PARTS",), x_kind="i8"),
            c("i8-128", "int", 130, 1024, 272, 0, "bf16", I8, 128, tune=i128, x_kind="i8"),
            c("i8-128", "int", 258, 1024, 272, 64, "f16", I8, 128, tune=i128, x_kind="i8"),
            c("i8-128", "introw", 130, 1024, 264, 32, "f32", I8, 128, tune=i128, x_kind="i8"),
            c("i8-128-codes", "w8a8", 130, 384, 272, 32, "f16", I8, 128, tune=i128, x_kind="i8"),
            c("i8-256", "int", 258, 1024, 272, 64, "bf16", I8, 256, tune=i256, x_kind="i8"),
            c("i8-256", "int", 258, 1024, 272, 64, "bf16", I8, 256, tune=i256 + ("AMAX_ATOMIC",), x_kind="i8"),
            c("i8-256", "int", 258, 1024, 272, 64, "bf16", I8, 256, tune=i256 + ("AMAX_PARTS",), x_kind="i8"),
            c("i8-256", "int", 258, 384, 264, 0, "f16", I8, 256, tune=i256, x_kind="i8"),
            c("i8-256", "introw", 258, 384, 260, 32, "f16", I8, 256, tune=i256, x_kind="i8"),
            c("i8-256-codes", "w8a8", 258, 1024, 272, 64, "bf16", I8, 256, tune=i256, x_kind="i8"),
            c("i8-256-codes", "w8a8", 258, 384, 272, 0, "f32", I8, 256, tune=i256, x_kind="i8")]
    # ---- pass-through fp16 activations on the fp16 main loop (a16_native), rank 0
    out += [c("smallm-f16x", "a16", 8, 320, 272, 0, "f16", S, 0, x_kind="f16"),
            c("tile64-f16x", "a16", 130, 320, 272, 0, "f16", T128, 64, x_kind="f16")]
    # ---- 256-row tiles, the whole forward: geometry A2276 of tests/_gemm256_cases.py (its file covers the product)
    out += [c("tile256", "mx", 4098, 320, 2276, 32, "f16", T256, 256, bias=True)]
    return out


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the group launch (lqer_linear_forward_group through SharedActivation): three Linears handed the same 3 tokens, each member against its
# own oracle value.  The members share x (xs) and draw everything else from their own ids.
GROUP_DTYPE = "f16"
GROUP = [Fx("mx", 3, 320, 272, 32, False, "group-x"), Fx("mx", 3, 320, 144, 32, False, "group-x"), Fx("opt", 3, 320, 272, 32, True, "group-x")]
FIXTURES = list(dict.fromkeys([c.fx for c in CASES] + GROUP))


def tuning_bits(case) -> int:
    from lqer_amd import _lib

    bits = 0
    for name in case.tune:
        bits |= getattr(_lib, "TUNE_" + name)
    return bits


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def _pcg(name):
    return np.random.Generator(np.random.PCG64(zlib.crc32(("exact_routes_" + name).encode())))


def _all_types(a):
    """The array as an fp32 tensor, asserted exact in fp16 and bf16 (and no fp16 subnormal)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    assert not bool(((t != 0) & (t.abs() < 2.0 ** -14)).any())
    return t


def _round8(a):
    """8 significant bits (bf16), nothing below fp16's smallest normal number."""
    t = torch.from_numpy(a.astype(np.float32)).bfloat16().float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t).numpy()


def _w_block(cfg, K):
    b = CONFIGS[cfg]["w_quantizer"]["block_size"][-1]
    return K if (b <= 0 or b > K) else b


def make_operands(fx):
    """x [M, K], W [N, K], A [K, r], B [r, N], bias [N] (None where the fixture has none) as CPU fp32 tensors."""
    M, K, N, r = fx.M, fx.K, fx.N, fx.r
    gx, g = _pcg("x-" + (fx.xs or fx_id(fx))), _pcg(fx_id(fx))
    x = gx.standard_normal((M, K)).astype(np.float32)
    if fx.cfg == "a16":
        x = np.clip(np.round(x * 32.0), -255, 255).astype(np.float32) / np.float32(32.0)  # fixed point: multiples of 2^-5
    x[:, 7] *= np.float32(OUTLIER)
    if M >= 8:
        x[5] = 0.0
    if M >= 3:
        x[1, 32:48] = 0.0
        x[M - 1, 0:16] = 0.0  # (a zero block in the ragged row tile)
    else:
        x[0, 32:48] = 0.0
    x = x if fx.cfg == "a16" else _round8(x)
    W = (0.02 * g.standard_normal((N, K))).astype(np.float32)
    wb = _w_block(fx.cfg, K)
    lo = -(SPREAD // 2)
    W *= np.repeat(np.exp2(g.integers(lo, lo + SPREAD, (N, (K + wb - 1) // wb))), wb, axis=1)[:, :K].astype(np.float32)
    W[2, 16:32] = 0.0
    W[N - 1] = 0.0  # (the last live column)
    W = _round8(W)
    A = B = b = None
    if r > 0:
        A = g.integers(-7, 8, (K, r)).astype(np.float32) * np.float32(2.0 ** -9)
        B = g.integers(-7, 8, (r, N)).astype(np.float32) * np.float32(2.0 ** -9)
    if fx.bias:
        b = np.round(0.01 * g.standard_normal(N) * 4096.0).astype(np.float32) / np.float32(4096.0)
    return tuple(None if a is None else _all_types(a) for a in (x, W, A, B, b))


def checksum(fx) -> int:
    """crc32 over the bytes of the fixture's operands (tests/test_exact_cases_cpu.py holds them to a table)."""
    crc = 0
    for t in make_operands(fx):
        if t is not None:
            crc = zlib.crc32(t.numpy().tobytes(), crc)
    return crc


# ---- grid units, bounds, ties -----------------------------------------------------------------------------------------------------------
def lsb_min(t):
    """The lowest set bit over the non-zero values of t (None if there is none): every value is a multiple of it."""
    a = np.abs(t.double().numpy()).ravel()
    a = a[a != 0]
    if a.size == 0:
        return None
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)
    return float(np.ldexp((mi & -mi).astype(np.float64), e - 53).min())


def _block_exps(v, qcfg):
    """Per element of v [rows, cols]: the shared exponent the oracle's block_fp quantizer `qcfg` gives its block; and the block length."""
    from oracle import lqer_oracle as O

    kw = {k: qcfg[k] for k in ("width", "exponent_width", "exponent_bias", "block_size", "skip_first_dim") if k in qcfg}
    _, _, exps = O.mxint_quantize(v.float(), decompose=True, **kw)
    L = O.infer_block_shape([1, v.shape[1]], list(qcfg["block_size"]))[-1]
    exps = exps.reshape(v.shape[0], -1)
    return exps.repeat_interleave(L, dim=1)[:, : v.shape[1]], exps, L


def ties(v64, qcfg):
    """How many elements of v64 the block_fp quantizer `qcfg` meets at an exact rounding tie (0 for another kind of quantizer): the scaled
    magnitude is an integer and a half below the clamp."""
    if qcfg.get("name") != "block_fp":
        return 0
    e, _, _ = _block_exps(v64, qcfg)
    mbits = qcfg["width"] - 1
    t = v64.abs() * torch.exp2((mbits - e).double())
    return int(((t - t.floor() == 0.5) & (t < 2 ** mbits - 1) & (v64.abs() > 1e-8)).sum())


@functools.lru_cache(maxsize=None)
def fixture(fx):
    """Computed once per fixture and left unchanged: the operands, the oracle's intermediates (fp32), the float64 value of every stage
    (the oracle's quantizers around float64 products), the grid unit and the exactness bound of each stage, and the tie counts."""
    from oracle import lqer_oracle as O

    x, W, A, B, b = make_operands(fx)
    qc = CONFIGS[fx.cfg] if fx.r > 0 else dict(CONFIGS[fx.cfg], name="flexible")
    out = O.lqer_linear_forward(x, W, b, A, B, qc, intermediates=True)
    d = lambda t: t.double()
    xq, wq = d(out["xq"]), d(out["wq"])
    main_abs = xq.abs() @ wq.abs().t()
    u_y = [lsb_min(xq) * lsb_min(wq)]
    y64 = xq @ wq.t()
    f = dict(fx=fx, x=x, W=W, A=A, B=B, b=b, qc=qc, out=out, units={}, bounds={}, ties={})
    if fx.bias:
        y64 = y64 + d(out["bq"])[None, :]
        main_abs = main_abs + d(out["bq"]).abs()[None, :]
        u_y.append(lsb_min(out["bq"]))
    if fx.r > 0:
        qs = O.resolve_linear_quantizers(qc)
        f["xA64"] = xq @ d(A)
        f["xAB64"] = d(out["xAq"]) @ d(B)
        y64 = y64 + d(out["xABq"])
        main_abs = main_abs + d(out["xABq"]).abs()
        u_y.append(lsb_min(out["xABq"]))
        f["units"]["xA"] = lsb_min(xq) * lsb_min(A)
        f["units"]["xAB"] = lsb_min(out["xAq"]) * lsb_min(B)
        f["bounds"]["xA"] = float((xq.abs() @ d(A).abs()).max()) / f["units"]["xA"] / 2.0 ** 24
        f["bounds"]["xAB"] = float((d(out["xAq"]).abs() @ d(B).abs()).max()) / f["units"]["xAB"] / 2.0 ** 24
        f["ties"] = {"A_out": ties(f["xA64"], qs["A_out"]), "B_out": ties(f["xAB64"], qs["B_out"])}
        f["qs"] = qs
    f["units"]["y"] = min(u for u in u_y if u is not None)
    f["bounds"]["y"] = float(main_abs.max()) / f["units"]["y"] / 2.0 ** 24
    f["y64"] = y64
    return f


def bounds_text(f) -> str:
    b = f["bounds"]
    return " ".join(f"{k} {b[k]:.4f}" for k in ("xA", "xAB", "y") if k in b)


# ---- modules ----------------------------------------------------------------------------------------------------------------------------
def make_module(fx, image="standard", flags=None, tuning=0):
    """The module of a fixture, unpacked and on the CPU, with the fixture's operands loaded."""
    import lqer_amd

    f = fixture(fx)
    if fx.r > 0:
        mod = lqer_amd.LinearFlexibleLqer(fx.K, fx.N, bias=fx.bias, q_config=f["qc"], l_config={"rank": fx.r})
    else:
        mod = lqer_amd.LinearFlexible(fx.K, fx.N, bias=fx.bias, q_config=f["qc"])
    for k, v in (flags or {}).items():
        assert hasattr(mod, k), k
        setattr(mod, k, v)
    sd = {"weight": f["W"].clone()}
    if fx.r > 0:
        sd.update(A=f["A"].clone(), B=f["B"].clone())
    if fx.bias:
        sd["bias"] = f["b"].clone()
    mod.load_state_dict(sd)
    mod.weight_image = image
    mod.tuning = tuning
    return mod


def host_desc(case):
    """The descriptor the GPU run will use, built without a GPU: the x format the packing is expected to choose is set by hand (the GPU
    test asserts that the packing chose it)."""
    mod = make_module(case.fx, flags=case.flags, tuning=tuning_bits(case)).to(DTYPES[case.dtype])
    mod._x_i8 = case.x_kind == "i8"
    mod._x_f16 = case.x_kind == "f16"
    return mod._desc()


def plan_answers(desc, M, dtype):
    """(route name, tile rows, lqer_decode_partials) from the library's host-only plan calls."""
    import ctypes as C

    from lqer_amd import _lib

    L = _lib.lib()
    code = {"f16": _lib.F16, "bf16": _lib.BF16, "f32": _lib.F32}[dtype]
    names = {_lib.ROUTE_SMALLM: S, _lib.ROUTE_TILE128: T128, _lib.ROUTE_TILE256: T256, _lib.ROUTE_I8: I8}
    route = L.lqer_gemm_route(C.byref(desc), M, code)
    assert route >= 0, L.lqer_last_error()
    return names[route], L.lqer_gemm_tile_rows(C.byref(desc), M, code), L.lqer_decode_partials(C.byref(desc), M)

"""Cases of the fused GEMM's 256-row tile kernel (lqer_amd/csrc/gemm_w4a8_m256.hip, k_lqer_gemm_m256) for tests/test_gpu_gemm256_exact.py:
the geometries, the inputs of the exact-product leg with their float64 reference, and the table of the side-path cases.

Geometries - the smallest the plan sends to LQER_ROUTE_TILE256 (M >= 512, more than 256 tiles of 128 x 256, at most 256 of 256 x 256):
  A      4098 x 2304   17 x 9 = 153 tiles (no multiple of 8: xcd_tile's tail), the last row tile with two live rows
  A2280  4098 x 2280   Np = 2304, ldy % 8 == 0: the last wave narrow (nb + 32 > N), the wave before it wide up to N - 8
  A2276  4098 x 2276   ldy % 8 != 0: every 16-bit store narrow; fp32: ldy % 4 == 0, the last float4 guarded by n + 3 < N
  B      514 x 16640   3 x 65 = 195 tiles: few row tiles, many column tiles

Exact-product leg: x and W are made once per K for M = 4098, N = 2304 (the ragged geometries take the first N rows of W: weight rows
are quantized independently), every value exact in fp32, fp16 and bf16 alike, so one oracle quantization and one float64 product serve
every geometry and output type of that K.  As in tests/_gemm128_cases.py: an outlier channel, an all-zero row, an all-zero block, a
power of two per (row, block of 16) of W - narrowed to what the exactness bound allows (see SPREAD, OUTLIER)."""
import functools
import zlib

import numpy as np
import torch

DEV = "cuda:0"
GEOM = {"A": (4098, 2304), "A2280": (4098, 2280), "A2276": (4098, 2276), "B": (514, 16640)}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
M_EXACT, N_EXACT = 4098, 2304
EXACT_KS = (64, 128, 192, 256, 320, 200, 1024)  # nk = 1 .. 5 (both prologue waits, every exit of the loop unrolled by 3), a zero-padded k-step, 16 steps

# The bound of the exact leg: with u = (smallest x step present) * (smallest W step present), every product is a multiple of u, and
# while sum |xq| |Wq| < 2^24 u every partial sum in any order is an integer below 2^24 in units of u - exact in fp32.  An 8-bit x code
# times a 4-bit W code is below 2^10 u at the smallest steps; K = 1024 terms of typical size take 2^16..2^17; what is left pays for the
# binades between the smallest and the typical steps.  x ~ N(0, 1): block maxima 0.5 .. 4.5, three binades that cannot be narrowed
# without giving up the normal draw.  That leaves the two knobs the bound is shaped with:
#   SPREAD   binades of the per-(row, block) power of two of W (tests/_gemm128_cases.py: 7)
#   OUTLIER  factor of the outlier channel 7 (there: 30) - its block's step is 2^ceil(log2(OUTLIER)) above the typical one, but it is one
#            block of 64, so it costs less than the spread of W does
# Measured on the CPU, max over the 4098 x 2304 outputs of sum |xq| |Wq| / u as a fraction of 2^24 (the largest sums are the outlier
# channel's; at K = 200 the half-filled last block of a row lowers the smallest x step by a binade or two):
#   SPREAD, OUTLIER      K = 1024    K = 200    K = 320    K = 64
#   7, 30                3.33                                          fails
#   6, 30                1.72                                          fails
#   5, 30                0.92        1.10       0.27       0.30        fails at K = 200
#   4, 30                0.49        0.55       0.14       0.15
#   5, 16                0.63        0.66       0.17       0.16        <- taken: five binades of weight exponents kept
SPREAD = 5
OUTLIER = 16.0


def route_of(mod, M, dtype):
    """(route, tile rows) the plan answers for this module, token count and tensor type."""
    import ctypes as C

    from lqer_amd import _lib

    d = mod._desc()
    dtc = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16, torch.float32: _lib.F32}[dtype]
    return _lib.lib().lqer_gemm_route(C.byref(d), M, dtc), _lib.lib().lqer_gemm_tile_rows(C.byref(d), M, dtc)


def _all_types(t):
    """t with every value exact in fp32, bf16 and fp16: 8 significant bits, nothing below fp16's smallest normal number."""
    t = t.bfloat16().float()
    t = torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
    assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
    return t


def make_exact_inputs(K):
    """x [4098, K], W [2304, K], bias [2304] (multiples of 2^-12) from numpy's PCG64 stream, seeded by K."""
    g = np.random.Generator(np.random.PCG64(zlib.crc32(f"gemm256_exact_k{K}".encode())))
    x = g.standard_normal((M_EXACT, K)).astype(np.float32)
    x[:, 7] *= np.float32(OUTLIER)
    x[5] = 0.0
    x[1, 32:48] = 0.0
    x[4097, 0:16] = 0.0  # (a zero block in the ragged row tile)
    W = (0.02 * g.standard_normal((N_EXACT, K))).astype(np.float32)
    lo = -(SPREAD // 2)
    W *= np.repeat(np.exp2(g.integers(lo, lo + SPREAD, (N_EXACT, (K + 15) // 16))), 16, axis=1)[:, :K].astype(np.float32)
    W[2, 16:32] = 0.0
    W[2279] = 0.0  # (the last live column of A2280)
    b = np.round(0.01 * g.standard_normal(N_EXACT) * 4096.0).astype(np.float32) / np.float32(4096.0)
    return _all_types(torch.from_numpy(x)), _all_types(torch.from_numpy(W)), _all_types(torch.from_numpy(b))


def _smallest_step(t, width, skip_first_dim):
    """The oracle's quantization of t in blocks of 16 along the last dim, and the smallest step 2^(e - mbits) among its blocks that hold
    a non-zero code."""
    from oracle import lqer_oracle as O

    q, codes, exps = O.mxint_quantize(t, width=width, block_size=[1, 16], skip_first_dim=skip_first_dim, decompose=True)
    R, K = t.shape
    nb = (K + 15) // 16
    c = torch.zeros(R, nb * 16, dtype=torch.int32)
    c[:, :K] = codes
    live = c.reshape(R, nb, 16).ne(0).any(-1)
    e = exps.reshape(R, nb)
    return q, 2.0 ** (int(e[live].min()) - (width - 1))


@functools.lru_cache(maxsize=None)
def exact_operands(K):
    """Per K, computed once and left unchanged: x, W, bias (CPU), u, the float64 product of the oracle's xq and Wq on the device (kept as
    fp32: below 2^24 u it is exact there, which is checked), and the bound max sum |xq| |Wq| / u as a fraction of 2^24.  The tests
    assert margin < 1 before they compare."""
    x, W, b = make_exact_inputs(K)
    xq, ux = _smallest_step(x, 8, True)
    Wq, uw = _smallest_step(W, 4, False)
    u = ux * uw
    xd, wd = xq.to(DEV).double(), Wq.to(DEV).double()
    ref64 = xd @ wd.t()
    margin = float((xd.abs() @ wd.abs().t()).max()) / u / 2.0 ** 24
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64) or margin >= 1.0  # (exact in fp32 whenever the bound holds; the tests assert the bound)
    return dict(x=x, W=W, b=b, u=u, ref32=ref32, margin=margin)


def exact_bias(K, N):
    """The oracle's b_quantizer(bias[:N]) (MXINT_Q: one block over the vector), whether it lies on the grid of u, and the bound with the
    bias as one more term: max sum |xq| |Wq| + max |bq|, over 2^24 u."""
    from bench import MXINT_Q
    from oracle import lqer_oracle as O

    op = exact_operands(K)
    bq = O.get_quantizer(MXINT_Q["b_quantizer"])(op["b"][:N].clone())
    units = bq.double() / op["u"]
    return bq, bool(torch.equal(units, units.round())), op["margin"] + float(bq.abs().max()) / op["u"] / 2.0 ** 24


# ---- side-path cases: (id, geometry, K, rank, config, bias, dtype) - config names resolved by side_config ---------------------------------
SIDE_CASES = [
    ("1-bout1-r16", "A", 320, 16, "mxint", True, "f16"),          # BOUT 1, one 16-deep slice of the side product
    ("2-ragged-kn", "A2280", 200, 32, "mxint", False, "bf16"),    # ragged K and N
    ("3-r64-narrow-f32", "A2276", 128, 64, "mxint", True, "f32"), # a whole 64-entry pass, narrow fp32 stores
    ("4-r80", "A", 192, 80, "mxint", False, "f16"),               # a second side_fetch pass with cols = 16
    ("5-r128-nk1", "A", 64, 128, "opt", True, "bf16"),            # two full passes, nk = 1, bias in blocks of 16
    ("6-bout0", "A", 256, 32, "pass", False, "f32"),              # BOUT 0
    ("7-bout2-row", "A2280", 320, 32, "row", False, "f16"),       # BOUT 2, row maxima from the pre-pass
    ("8-int-limbs", "A", 384, 32, "int", False, "f16"),           # BOUT 2, unquantized A / B: two bf16 limbs of B
    ("8-int-limbs-f32", "A", 128, 32, "int", False, "f32"),       # ... three limbs (fp32 tensors), two k-steps
    ("9-integer-bout", "A", 128, 32, "integer", False, "f16"),    # fixed-point B_out: bout_amax == nullptr
    ("10-many-columns", "B", 128, 32, "mxint", True, "bf16"),     # 65 column tiles
    ("11-f16x", "A", 256, 32, "a16", False, "f16"),               # pass-through fp16 activations on the fp16 MFMA: LQER_F16X
    ("12-steady-state", "A", 1024, 32, "mxint", False, "f16"),    # 16 k-steps: the ring's steady state
]


def side_config(name):
    from bench import A16_Q, INT_Q, MXINT_Q, OPT_Q, _bfp

    if name == "integer":  # as tests/test_gpu_integer.py builds it: A_out and B_out fall back to the integer x quantizer
        return dict(name="flexible_lqer", is_ptq=True, default=False, x_quantizer=dict(name="integer", width=8, frac_width=4),
                    w_quantizer=_bfp(4, [1, 16], False), b_quantizer=dict(name="integer", width=8, frac_width=6))
    return {"mxint": MXINT_Q, "opt": OPT_Q, "pass": dict(MXINT_Q, B_out_quantizer={"name": "passthrough"}),
            "row": dict(MXINT_Q, B_out_quantizer=_bfp(8, [1, -1], True)), "int": INT_Q, "a16": A16_Q}[name]


@functools.lru_cache(maxsize=None)
def side_case(cid):
    """The module of a side-path case on the device, its input there, and the CPU operands (for the oracle).  A and B are on the 8-bit
    MXINT grid except in the INT configuration, whose template leaves them unquantized."""
    import lqer_amd
    from bench import make_case

    _, geom, K, r, cfg, bias, dt = next(c for c in SIDE_CASES if c[0] == cid)
    M, N = GEOM[geom]
    dtype = DTYPES[dt]
    qc = side_config(cfg)
    case = make_case(M, K, N, r, seed=zlib.crc32(cid.encode()) % 1000, bias=bias, quantize_ab=cfg != "int")
    x, W, A, B = case[:4]
    mod = lqer_amd.LinearFlexibleLqer(K, N, bias=bias, q_config=qc, l_config={"rank": r})
    if cfg == "int":
        mod.a8_native = False  # per-token 8-bit activations stay on the bf16 kernels (by default they take the int8 MFMA route at every M >= 128)
    sd = {"weight": W, "A": A, "B": B}
    if bias:
        sd["bias"] = case[4]
    mod.load_state_dict(sd)
    mod = mod.to(DEV).to(dtype)
    return mod, x.to(dtype).to(DEV), dict(x=x, W=W, A=A, B=B, b=case[4] if bias else None, qc=qc, M=M, N=N, K=K, r=r, dtype=dtype)


def slice_starts(M):
    """Starts of the 256-row slices that cover rows 0 .. M - 1: consecutive, the last one moved back to end at M (a remainder of fewer
    than 65 rows alone would take the small-M kernel, not the 128-row tiles)."""
    s = list(range(0, M - 255, 256))
    if s[-1] + 256 < M:
        s.append(M - 256)
    return s

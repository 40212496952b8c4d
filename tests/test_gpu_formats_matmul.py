"""lqer_matmul_q (lqer_amd.matmul_flexible: x quantized in the GEMM's load path, y through a bf16 image) with DIFFERENT narrow
block_fp formats for x and y (tests/_formats.py): blocks of 16 on both operands, and one operand in blocks of 32 or whole rows
(the route through the standalone quantizer's image).  Shapes [4, 70, 48] x [4, 48, 150].

Exact leg: x = integer mantissas times 2^a per row, y = integer mantissas times 2^b per block of columns (blocks run along the last
dim of y, which is not the contraction dim); every block holds the width's largest mantissa and a, b walk the formats' ladders, so
both clamps are met (asserted on the oracle, on the CPU, first) and every product of one output element lies on one grid: the sums
are exact in any order (below 2^24 grid steps, asserted), and the product must equal oracle.matmul_flexible rounded to the dtype and
the two-step GPU route (both operands through the standalone quantizer, torch.matmul) - value for value, no tolerance.
Random leg: inputs on the ladder against the two-step route at tools/fuzz_matmul.py's bars (1e-3 fp16, 6e-3 bf16, 1e-6 fp32).
"""
import pytest
import torch

import _formats as F
from oracle import lqer_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
BARS = {"f16": 1e-3, "bf16": 6e-3, "f32": 1e-6}
# (x pair, x block, y pair, y block)
CASES = [(("e4", 8), 16, ("e3b6", 8), 16), (("e3b6", 4), 16, ("e4", 4), 16), (("e3bm2", 8), 16, ("e2", 6), 16), (("e1", 6), 16, ("e3bm2", 3), 16),
         (("e2", 3), 16, ("e1", 8), 16), (("e5b20", 8), 16, ("e8b120", 4), 16), (("e8", 2), 16, ("e5b20", 6), 16), (("e8b120", 6), 16, ("e8", 8), 16),
         (("e4", 8), 32, ("e3b6", 4), 16), (("e3bm2", 4), 16, ("e4", 8), 32), (("e2", 8), -1, ("e4", 6), 16)]
B, S1, K, S2 = 4, 70, 48, 150


def _params():
    out = []
    for c in CASES:
        for dt in DTYPES:
            if dt == "f16" and not (c[0][0] in F.FP16_IDS and c[2][0] in F.FP16_IDS):
                continue
            out.append(pytest.param(c, dt, id=f"x{F.pair_id(c[0])}b{c[1]}-y{F.pair_id(c[2])}b{c[3]}-{dt}"))
    return out


def _qc(c):
    (fx, wx), bx, (fy, wy), by = c
    xq, yq = F.cfg(fx, wx, [1, bx], True), F.cfg(fy, wy, [1, by], True)
    return dict(name="flexible", default=xq, x_quantizer=xq, w_quantizer=yq)


def _two_step(x, y, qc):
    from lqer_amd import functional

    return torch.matmul(functional._quantize(x, dict(qc["x_quantizer"])).float(), functional._quantize(y, dict(qc["w_quantizer"])).float())


@pytest.mark.parametrize("c,dt", _params())
def test_exact_product(c, dt):
    import lqer_amd

    (fx, wx), bx, (fy, wy), by = c
    dtype = DTYPES[dt]
    qc = _qc(c)
    g = torch.Generator().manual_seed(13)
    xm, ym = 2 ** (wx - 1) - 1, 2 ** (wy - 1) - 1
    ex = F.ladder_e(fx, dtype, B * S1, g)
    x = (F.ints(B * S1, K, xm, bx, g) * torch.pow(2.0, (ex - F.lg(xm)).float())[:, None]).reshape(B, S1, K)
    Ly = S2 if by <= 0 else by
    nby = -(-S2 // Ly)
    ey = F.ladder_e(fy, dtype, B * nby, g).reshape(B, 1, nby).repeat_interleave(Ly, dim=2)[:, :, :S2]
    y = F.ints(B * K, S2, ym, by, g).reshape(B, K, S2) * torch.pow(2.0, (ey - F.lg(ym)).float())
    x, y = x.to(dtype), y.to(dtype)
    assert bool(torch.isfinite(x.float()).all() and torch.isfinite(y.float()).all())
    F.assert_covered(x.reshape(B * S1, K), fx, dict(qc["x_quantizer"]), dtype)
    if by > 0:  # (one block per row of y: one exponent per batch element - three classes over four elements, not 15 % of anything)
        F.assert_covered(y.reshape(B * K, S2), fy, dict(qc["w_quantizer"]), dtype)
    # the declared difference: a non-zero |x| <= 1e-8 is kept by the reference and flushed to 0 by every image of the HIP path (the low
    # rungs of e5b20's ladder reach it) - the expected product is the oracle's on the inputs with exactly those elements at 0
    flush = lambda t: torch.where(t.abs() <= 1e-8, torch.zeros_like(t), t)
    xo, yo = flush(x.float()), flush(y.float())
    xq = O.get_quantizer(qc["x_quantizer"])(xo)
    yq = O.get_quantizer(qc["w_quantizer"])(yo)
    steps = max(F.exact_steps(xq[i], yq[i]) for i in range(B))
    assert steps < 2.0 ** 24, f"the product needs {steps:.3g} grid steps: not exact in fp32"
    ref = O.matmul_flexible(xo, yo, qc)
    got = lqer_amd.matmul_flexible(x.to(DEV), y.to(DEV), qc)
    assert got.dtype == dtype
    F.assert_same_finite(got.cpu().reshape(B * S1, S2), ref.reshape(B * S1, S2), dtype, "lqer_matmul_q against the oracle")
    # (the standalone quantizer's `deq` keeps the pass-through elements, the fused kernel's images flush them: the same inputs at 0)
    two = _two_step(flush(x).to(DEV), flush(y).to(DEV), qc).to(dtype)
    fin = torch.isfinite(two.float())
    assert torch.equal(got.float()[fin], two.float()[fin]), "fused product differs from the two-step route"


# (e8b120's ladder lives at 2^108 .. 2^120, where no product is finite: the exact leg covers that format)
@pytest.mark.parametrize("c,dt", [p for p in _params() if "e8b120" not in (p.values[0][0][0], p.values[0][2][0])])
def test_random_ladder_vs_two_step(c, dt):
    import lqer_amd

    (fx, wx), bx, (fy, wy), by = c
    dtype = DTYPES[dt]
    qc = _qc(c)
    x = F.ladder(fx, dtype, B * S1, K, bx, seed=90).reshape(B, S1, K)
    y = F.ladder(fy, dtype, B * K, S2, by, seed=91).reshape(B, K, S2)
    F.assert_covered(x.reshape(B * S1, K), fx, dict(qc["x_quantizer"]), dtype)
    F.assert_covered(y.reshape(B * K, S2), fy, dict(qc["w_quantizer"]), dtype)
    # y as the transposed view of a [S2, K] tensor for every other case (the Q K^T call site)
    yd = y.to(DEV)
    if CASES.index(c) % 2:
        yd = y.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    got = lqer_amd.matmul_flexible(x.to(DEV), yd, qc).float()
    ref = _two_step(x.to(DEV), yd, qc)
    fin = torch.isfinite(ref.to(dtype).float()) & torch.isfinite(got)
    assert float(fin.float().mean()) >= 0.25  # (fp16: products of two rungs above emax overflow; the bar runs over the rest)
    err = float((got[fin] - ref[fin]).norm() / ref[fin].norm().clamp_min(1e-30))
    print(f"matmul_q {c} {dt}: rel-L2 vs the two-step route {err:.2e} over {float(fin.float().mean()):.2f} of the outputs")
    assert err <= BARS[dt]

"""The activation side on its own (lqer_quantize_act_xa: the image of Q_x(x) and xAq = A_out(Q_x(x) A)) with a narrow exponent field
in A_out (tests/_formats.py), compared directly - not through the GEMM behind it, as tests/test_gpu_formats_linear.py does.

A_out keeps width 8 and varies the exponent field only, as in the Linear tests.  x runs under the control format so that the rows'
scales, and with them the block exponents of x A, walk A_out's ladder: below emin, inside, above emax.  Every case asserts on the
oracle, before its first GPU call, that each class A_out's format can reach holds 15 % of the non-zero blocks of x A.

Exact: x integer mantissas up to 127 times 2^a(row), A integer-valued in [-3, 3] times one power of two.  x A is then exact in any
summation order, so both outputs must be the oracle's bit for bit, with the declared flush of |v| <= 1e-8 (the reference keeps such
an element unquantized, every packed image holds 0).  Rank 32 at M = 100 is the 64-row kernel, rank 128 at M = 520 the 128-row one.

Random: one ordinary case per format - uniform rows on the ladder, an 8-bit MXINT A - through tests/_envelope.py's criterion for a
sum whose order differs from the reference's, given the format's emin / emax.
"""
import ctypes as C
import math

import pytest
import torch

import _formats as F
from _envelope import envelope_check
from oracle import lqer_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
A_OUT = ("e4", "e2", "e1", "e3b6", "e3bm2", "e5b20")  # every format of the table with a clamp inside fp32


def _flush(x, q):
    return torch.where(x.abs() <= 1e-8, torch.zeros_like(q), q)


def _act_xa(x, A, fa, r):
    """lqer_quantize_act_xa through the C ABI -> (image of xq [M, K] as fp32, xAq [M, r] as fp32), both on the CPU."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    M, K = x.shape
    xf = ops.make_qfmt(F.cfg("e8", 8), "x")
    wf = ops.make_qfmt(F.cfg("e8", 4, [1, 16], False), "w")
    af = ops.make_qfmt(F.cfg(fa, 8), "A_out")
    desc = _lib.LinearDesc(K, 256, r, 0, xf, wf, xf, af, xf)
    a_t, _, a_limbs, _ = ops.pack_lowrank(A.to(DEV), torch.zeros(r, 256, device=DEV))
    xd = x.to(DEV)
    Mp, Kp, rp = L.lqer_padded_m(M), L.lqer_padded_k(K), L.lqer_padded_r(r)
    xq = torch.full((Mp, Kp), 7.0, dtype=torch.bfloat16, device=DEV)
    xaq = torch.full((Mp, rp), 7.0, dtype=torch.bfloat16, device=DEV)
    nscr = L.lqer_lowrank_xa_scratch_bytes(C.byref(desc), M)
    scr = torch.empty(max(nscr, 16), dtype=torch.uint8, device=DEV)
    _lib.check(L.lqer_quantize_act_xa(C.byref(desc), xd.data_ptr(), ops.dtype_code(xd), M, K, a_t.data_ptr(), a_limbs, xq.data_ptr(),
                                      xaq.data_ptr(), scr.data_ptr(), nscr, None), "quantize_act_xa")
    torch.cuda.synchronize()
    return xq[:M, :K].float().cpu(), xaq[:M, :r].float().cpu()


CASES = [pytest.param(fa, M, r, dt, id=f"A{fa}-M{M}-r{r}-{dt}") for fa in A_OUT for M, r in ((100, 32), (520, 128)) for dt in DTYPES
         if dt != "f16" or fa in F.FP16_IDS]


@pytest.mark.parametrize("fa,M,r,dt", CASES)
def test_xq_and_xaq_exact(fa, M, r, dt):
    dtype, K = DTYPES[dt], 320
    g = torch.Generator().manual_seed(17)
    ea = F.ladder_e(fa, dtype, M, g)
    pA = min(0, int(ea.min()) + 12)  # (e5b20: A carries the low powers of two, x stays above the pass-through range)
    A = torch.randint(-3, 4, (K, r), generator=g).float() * 2.0 ** pA
    lg_xa = math.ceil(math.log2(127 * 2 * math.sqrt(K)))
    x = (F.ints(M, K, 127, 16, g) * torch.pow(2.0, (ea - lg_xa - pA).float())[:, None]).to(dtype)
    x[M // 2, :16] = 0
    assert torch.equal(x.float().to(dtype).float(), x.float()) and not bool(((x.float() != 0) & (x.float().abs() <= 1e-8)).any())
    want_xq = F.oracle_q(x, F.cfg("e8", 8))
    xA = want_xq @ A
    F.assert_covered(xA, fa, F.cfg(fa, 8), dtype)
    assert F.exact_steps(want_xq, A) < 2.0 ** 24
    want_xaq = _flush(xA, F.oracle_q(xA, F.cfg(fa, 8)))
    xq, xaq = _act_xa(x, A, fa, r)
    assert torch.equal(xq, want_xq), f"xq: {(xq != want_xq).sum().item()} of {xq.numel()} differ"
    bad = (xaq != want_xaq).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(xaq, want_xaq), f"xAq: {(xaq != want_xaq).sum().item()} of {xaq.numel()} differ, in rows {bad[:12]}"


@pytest.mark.parametrize("fa", A_OUT)
def test_random_side_path_inside_the_envelope(fa):
    dtype = torch.float16 if fa in F.FP16_IDS else torch.bfloat16
    M, K, r = 300, 1088, 32
    g = torch.Generator().manual_seed(19)
    ea = F.ladder_e(fa, dtype, M, g)
    pA = max(0, -int(ea.min()) - 12)  # (e5b20: A carries 2^-pA, so that x stays above the pass-through range)
    A = O.mxint_quantize(0.01 * torch.randn(K, r, generator=g), width=8, block_size=[16, 1], skip_first_dim=False) * 2.0 ** -pA
    A = torch.where(A.abs() <= 1e-8, torch.zeros_like(A), A)
    # the rows' scales: 2^(a - shift), shift the typical block exponent of x A for rows at 2^0 (measured on the draw itself)
    x0 = torch.rand(M, K, generator=g) * 2 - 1
    shift = int(O.ceil_log2_f32((x0 @ A)[:, :16].abs().amax(dim=1)).median())
    x = (x0 * torch.pow(2.0, (ea - shift).float())[:, None]).to(dtype)
    x[5] = 0
    want_xq = _flush(x.float(), F.oracle_q(x, F.cfg("e8", 8)))
    s64 = want_xq.double().numpy() @ A.double().numpy()
    F.assert_covered(torch.from_numpy(s64).float(), fa, F.cfg(fa, 8), dtype)
    xq, xaq = _act_xa(x, A, fa, r)
    assert torch.equal(xq, want_xq)
    emin, emax = F.e_range(fa)
    bad = envelope_check(s64, xaq.numpy(), 16, 7, max(16.0, math.sqrt(K)), emin, emax)
    assert bad == 0, f"{bad} row-blocks of xAq outside the fp32-summation envelope under {fa}"
    assert envelope_check(s64, xaq.numpy(), 16, 7, max(16.0, math.sqrt(K))) > 0, "the case meets no clamp: the unclamped criterion holds too"

"""lqer_qerr_matmul (lqer_amd/csrc/qerr_mm.hip; include/lqer_hip.h "quantization-error products") and the subspace-iteration
approximator built on it (lqer_amd.approximate.lqer_factors, method="subspace"), against float64 products on the CPU with E from the
oracle's quantizer."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lqer_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def w_cfg_of(block, width, rows=1):
    return dict(name="block_fp", width=width, exponent_width=8, exponent_bias=None, block_size=[rows, block], skip_first_dim=False)


def make_w(N, K, dtype, ldw=None):
    """0.02 randn, one column x 20, a few exact zeros and |w| <= 1e-8 entries; the values of `dtype`, as a view of row stride ldw."""
    g = torch.Generator().manual_seed(100 * N + K)
    W = 0.02 * torch.randn(N, K, generator=g)
    W[:, min(5, K - 1)] *= 20
    W.view(-1)[::7] = 0.0
    W.view(-1)[3::11] = 5e-9
    buf = torch.zeros(N, ldw or K, dtype=dtype)
    buf[:, :K] = W.to(dtype)
    return buf[:, :K]


# trans, (N, K), block, width, dtype, L, scale, (ldw - K, ldy - L)
CASES = [
    (0, (48, 176), 16, 4, "f16", 48, False, (0, 0)),
    (1, (48, 176), 16, 4, "f16", 48, True, (0, 0)),
    (0, (200, 328), 32, 8, "bf16", 144, True, (0, 0)),
    (1, (200, 328), 128, 4, "f32", 144, False, (0, 0)),
    (0, (1, 16), 16, 8, "f32", 8, False, (0, 0)),
    (1, (1, 16), 16, 4, "bf16", 8, True, (0, 0)),
    (0, (37, 40), 32, 4, "f16", 8, True, (0, 0)),
    (1, (37, 40), 128, 8, "f16", 48, False, (0, 0)),
    (0, (200, 328), 128, 4, "f16", 48, False, (0, 0)),
    (1, (200, 328), 32, 8, "bf16", 8, True, (0, 0)),
    (0, (37, 40), 16, 4, "f32", 144, True, (3, 5)),
    (1, (48, 176), 16, 8, "f16", 48, True, (8, 1)),
]


@pytest.mark.parametrize("trans,shape,block,width,dtype,L,with_scale,pads", CASES)
def test_product_against_float64(trans, shape, block, width, dtype, L, with_scale, pads):
    """|Y - Y64| <= (n + 8) 2^-23 (|E_s| |X|) elementwise, n the contraction length: the fp32 accumulation bound (any order), slack 2."""
    from lqer_amd import ops

    (N, K), cfg = shape, w_cfg_of(block, width)
    W = make_w(N, K, DT[dtype], K + pads[0])
    g = torch.Generator().manual_seed(7)
    X = torch.randn(N if trans else K, L, generator=g)
    s = (0.5 + torch.rand(K, generator=g)) if with_scale else None
    rows = K if trans else N
    out = torch.full((rows, L + pads[1]), -7.0, device=DEV)
    Y = ops.qerr_matmul(W._base.to(DEV)[:, :K], cfg, X.to(DEV), trans, None if s is None else s.to(DEV), out=out[:, :L]).cpu().double()
    Es = (W.float() - O.get_quantizer(cfg)(W.float())).t().double() * (1.0 if s is None else s.double()[:, None])  # [K, N]
    op = Es if trans else Es.t()
    ref, bound = op @ X.double(), (op.shape[1] + 8) * 2.0 ** -23 * (op.abs() @ X.double().abs())
    excess = float(((Y - ref).abs() - bound).max())
    print(f"max |Y - Y64| {float((Y - ref).abs().max()):.3e}, max bound {float(bound.max()):.3e}, excess {excess:.3e}")
    assert excess <= 0.0
    assert torch.all(out[:, L:] == -7.0)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("shape,block,dtype", [((200, 328), 32, "f16"), ((37, 40), 128, "bf16"), ((48, 176), 16, "f32")])
def test_fused_source_equals_dense_source(trans, shape, block, dtype):
    """The in-register quantizer is the library's: the fused call and the dense call on E = W - quantize_mxint(W) agree bit for bit."""
    from lqer_amd import ops

    (N, K), cfg = shape, w_cfg_of(block, 4)
    W = make_w(N, K, DT[dtype]).to(DEV)
    X = torch.randn(N if trans else K, 48, generator=torch.Generator().manual_seed(1)).to(DEV)
    s = (0.5 + torch.rand(K, generator=torch.Generator().manual_seed(2))).to(DEV)
    E = W.float() - ops.quantize_mxint(W.float(), ops.make_qfmt(cfg, "w"), want=("deq",))["deq"]
    assert float(E.abs().max()) > 0
    assert torch.equal(ops.qerr_matmul(W, cfg, X, trans, s), ops.qerr_matmul(E, None, X, trans, s))


@pytest.mark.parametrize("trans", [0, 1])
def test_determinism_and_extents(trans):
    """Equal bits over NaN-filled workspaces; sentinels in the row gaps of Y and behind its last element stay."""
    from lqer_amd import ops

    N, K, L, ldy = 200, 328, 48, 53
    cfg, W = w_cfg_of(16, 4), make_w(200, 328, torch.float16).to(DEV)
    X = torch.randn(N if trans else K, L, generator=torch.Generator().manual_seed(4)).to(DEV)
    rows, outs = (K if trans else N), []
    for _ in range(2):
        nbytes = ops._lib.lib().lqer_qerr_matmul_workspace_bytes(N, K, L, trans)
        ops.workspace(torch.device(DEV), nbytes)[: nbytes // 4 * 4].view(torch.float32).fill_(float("nan"))
        flat = torch.full(((rows - 1) * ldy + L + 64,), -7.0, device=DEV)
        ops.qerr_matmul(W, cfg, X, trans, None, out=flat[: rows * ldy - (ldy - L)].as_strided((rows, L), (ldy, 1)))
        outs.append(flat.cpu())
    assert torch.equal(outs[0], outs[1])
    body = outs[0][: (rows - 1) * ldy + L]
    gaps = torch.nn.functional.pad(body, (0, ldy - L)).view(rows, ldy)[:, L:]
    assert torch.all(gaps[:-1] == -7.0) and torch.all(outs[0][(rows - 1) * ldy + L:] == -7.0)
    assert torch.isfinite(body).all() and float(body.view(-1)[:L].abs().max()) > 0


@pytest.mark.parametrize("with_scale,w_block", [(False, [1, 16]), (True, [1, 16]), (False, [8, 16]), (True, [8, 16])])
def test_subspace_factors(with_scale, w_block):
    """lqer_factors(method="subspace") leaves the error the oracle's full SVD leaves (2e-3 relative, the margin between routes of
    tests/test_gpu_parity.py's approximator test); [8, 16] weight tiles take the dense source.  The factors lie on the 8-bit grid."""
    from lqer_amd.approximate import lqer_factors

    torch.manual_seed(3)
    N, K, r = 192, 160, 16
    W = 0.02 * torch.randn(N, K)
    W[:, 5] *= 20
    w_cfg = dict(name="block_fp", width=4, exponent_width=8, exponent_bias=None, block_size=w_block, skip_first_dim=False)
    ab_cfg = dict(name="block_fp", width=8, exponent_width=8, exponent_bias=None, block_size=[16, 1], skip_first_dim=False)
    scale = (0.5 + torch.rand(K)) if with_scale else None
    sd = scale.to(DEV) if with_scale else None
    A, B = lqer_factors(W.to(DEV), w_cfg, r, ab_cfg, ab_cfg, sd, method="subspace", seed=3)
    A2, B2 = lqer_factors(W.to(DEV), w_cfg, r, ab_cfg, ab_cfg, sd, method="subspace", seed=3)
    assert torch.equal(A, A2) and torch.equal(B, B2)
    Ao, Bo = O.lqer_factors(W, w_cfg, r, ab_cfg, ab_cfg, scale)
    assert A.shape == (K, r) and B.shape == (r, N)
    err_t = (W - O.get_quantizer(w_cfg)(W)).t()
    e_sub = float((err_t - A.cpu() @ B.cpu()).norm() / err_t.norm())
    e_ora = float((err_t - Ao @ Bo).norm() / err_t.norm())
    print(f"e_sub {e_sub:.6f} e_ora {e_ora:.6f} rel {abs(e_sub - e_ora) / e_ora:.2e}")
    assert abs(e_sub - e_ora) <= 2e-3 * e_ora, (e_sub, e_ora)
    for t in (A.cpu(), B.cpu()):
        blk = t.t().reshape(t.shape[1], -1, 16)
        step = 2.0 ** torch.ceil(torch.log2(blk.abs().amax(-1, keepdim=True).clamp_min(1e-30))) / 128
        assert torch.all((blk / step - torch.round(blk / step)).abs() < 1e-4)

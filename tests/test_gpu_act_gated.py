"""Gated MLP inside the down projection's activation side (lqer_amd/csrc/act_gated.hip: lqer_quantize_act_xa_gated,
lqer_linear_forward_gated, LinearFlexibleLqer.forward_gated, quantize_model(fuse_mlp=True)) against a plain fp64 reference of
    s = round_dt(g / (1 + exp(-g))),  h = round_dt(s * u)
followed by the oracle's quantizers: the activation image bit for bit, h_q A inside the summation-order envelope and bit-stable, the
forward at the parity gate, and a tiny Llama with and without the fusion.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from _envelope import envelope_check  # noqa: E402
from oracle import lqer_oracle as O  # noqa: E402

DEV = "cuda:0"
N = 256
F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 1e-3, BF16: 5e-3}  # tests/test_gpu_parity.py, per output dtype (1e-3 for fp16)


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return __import__("lqer_amd")


def _inputs(M, K, dt, seed):
    """(g, u) in dt: g uniform over [-20, 20] mixed with randn (both SiLU tails, fp16-subnormal results), u = randn with three outlier
    channels x30, an all-zero block, a block at an extreme exponent - and g = 0 wherever fp32 cannot be asked for the bits of silu."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.where(torch.rand(M, K, generator=gen) < 0.5, 40 * torch.rand(M, K, generator=gen) - 20, torch.randn(M, K, generator=gen))
    u = torch.randn(M, K, generator=gen)
    for c in (7, 100, K - 3):
        u[:, c] *= 30.0
    g[0, 16:32] = 0.0
    sign = torch.where(torch.arange(16) % 3 == 0, -1.0, 1.0)
    g[0, 48:64] = 10.0 + torch.arange(16) / 4  # h at 2^-121 (bf16: the quantizer's element routine) / at fp16's top
    u[0, 48:64] = sign * (2.0 ** -125 if dt == BF16 else 2400.0) * (1 + torch.arange(16) / 16)
    g, u = g.to(dt), u.to(dt)
    s64 = g.double() / (1 + torch.exp(-g.double()))
    mask = (s64 * (1 - 2.0 ** -18)).to(dt) != (s64 * (1 + 2.0 ** -18)).to(dt)
    assert float(mask.float().mean()) < 0.05
    return torch.where(mask, torch.zeros_like(g), g), u


def _h_ref(g, u, act):
    dt = g.dtype
    s = (g.double() / (1 + torch.exp(-g.double()))).to(dt) if act == "silu" else torch.relu(g)
    return s if u is None else (s.double() * u.double()).to(dt)


CASES = [
    # M, K, rank, dtype, operands, x width
    (1, 512, 32, F16, "separate", 8),      # below a row group, one slab (seven waves idle)
    (8, 640, 16, F16, "halves", 8),        # exactly one row group, a part-filled second slab, one rank tile
    (13, 4608, 64, BF16, "separate", 8),   # a ragged second group, wave 0 carries a second slab, four rank tiles
    (24, 4608, 32, F16, "halves", 4),      # several groups, a narrow x / A_out format
    (13, 640, 0, BF16, "halves", 8),       # rank 0: the image alone
    (24, 512, 32, BF16, "relu", 4),        # up = None with relu
    (13, 4608, 16, F16, "relu", 8),
]


@pytest.mark.parametrize("M,K,r,dt,operands,xw", CASES)
def test_gated_activation_side_and_forward(lq, M, K, r, dt, operands, xw):
    from bench import MXINT_Q, _bfp, make_weights
    from lqer_amd import _lib, ops

    qc = dict(MXINT_Q, x_quantizer=_bfp(xw, [1, 16], True))
    act = "relu" if operands == "relu" else "silu"
    g, u = _inputs(M, K, dt, seed=M + K + r)
    if operands == "relu":
        u = None
    W, A, B = make_weights(torch.Generator().manual_seed(K + r), K, N, max(r, 1))
    if r:
        mod = lq.LinearFlexibleLqer(K, N, bias=False, q_config=qc, l_config={"rank": r})
        mod.load_state_dict({"weight": W, "A": A, "B": B})
    else:
        mod = lq.LinearFlexible(K, N, bias=False, q_config=dict(qc, name="flexible"))
        mod.load_state_dict({"weight": W})
    mod = mod.to(DEV).to(dt)
    mod._pack()
    p, desc, L = mod._packed, mod._desc(), _lib.lib()
    assert desc.rank == r and (not r or "a_t_b16" in p)
    gd, ud = g.to(DEV), None if u is None else u.to(DEV)
    if operands == "halves":  # the two halves of one [M, 2K] tensor
        gd, ud = torch.cat([g, u], dim=1).to(DEV).split(K, dim=1)
    Kp, Mp, rp = L.lqer_padded_k(K), L.lqer_padded_m(M), L.lqer_padded_r(r) if r else 0
    xaq_off = (Mp * Kp * 2 + 255) // 256 * 256
    (a_t, b_t), st = (p["a_t_b16"].data_ptr(), p["b_t"].data_ptr()) if r else (None, None), torch.cuda.current_stream().cuda_stream
    lead = (C.byref(desc), gd.data_ptr(), None if ud is None else ud.data_ptr(), _lib.ACT_RELU if act == "relu" else _lib.ACT_SILU,
            ops.dtype_code(gd), M, gd.stride(0), K if ud is None else ud.stride(0))

    def read(ws):
        torch.cuda.synchronize()
        img = ws[: Mp * Kp * 2].view(torch.bfloat16).view(Mp, Kp)[:M].clone()
        return img, ws[xaq_off: xaq_off + Mp * rp * 2].view(torch.bfloat16).view(Mp, rp)[:M].float().cpu() if r else None

    ws = torch.full((ops.linear_sizes(desc, M).workspace,), 0x5A, dtype=torch.uint8, device=DEV)
    y = torch.empty(M, N, dtype=dt, device=DEV)
    _lib.check(L.lqer_linear_forward_gated(*lead, p["w"].data_ptr(), a_t, b_t, -2, p.get("b_limbs", 0), None, y.data_ptr(), N, ws.data_ptr(),
                                           ws.numel(), st), "linear_forward_gated")
    img, xa = read(ws)
    ws2 = torch.full_like(ws, 0xA5)
    _lib.check(L.lqer_quantize_act_xa_gated(*lead, a_t, -2, ws2.data_ptr(), ws2.data_ptr() + xaq_off if r else None, st), "quantize_act_xa_gated")
    img2, xa2 = read(ws2)
    # (1) the image: the oracle's quantizer applied to h_ref, bit for bit (|h| <= 1e-8 flushed in images), zeros in the padded k
    h = _h_ref(g, u, act).float()
    ref = O.get_quantizer(qc["x_quantizer"])(h)
    assert torch.equal(img[:, :K].float().cpu(), torch.where(h.abs() <= 1e-8, torch.zeros_like(ref), ref))
    assert Kp == K or float(img[:, K:].float().abs().max()) == 0.0
    # (2) h_q A inside the envelope of the exact sum of exact products; a second call (the split entry): identical bits
    assert torch.equal(img.view(torch.int16), img2.view(torch.int16))
    if r:
        s64 = img[:, :K].double().cpu().numpy() @ A.to(dt).double().numpy()
        assert envelope_check(s64, xa[:, :r].numpy(), 16, xw - 1, max(16.0, math.sqrt(K))) == 0
        assert torch.equal(xa, xa2)
    # (3) the forward against the oracle's on h_ref
    c = lambda t: t.to(dt).float()
    want = O.lqer_linear_forward(h, c(W), None, c(A) if r else None, c(B) if r else None, qc)
    err = float((y.float().cpu() - want).norm() / want.norm())
    print(f"rel-L2 of y against the oracle: {err:.3e}")
    assert err <= TOL[dt]


def test_tiny_llama_with_and_without_the_fusion(lq, monkeypatch):
    """fuse_mlp=True against fuse_mlp=False on the fp16 model of tests/test_model_swap.py: the same exact products, h differs by the last
    bit of silu on rounding boundaries of fp16 - that file's tolerance for two fp16 routes of one model (3e-3).  48 tokens: the fused
    entry is switched on below the token count from which the module takes it by default."""
    from bench import MXINT_Q
    from lqer_amd.models import load_low_rank_dict, quantize_model
    from test_model_swap import _ab_dict, _tiny_llama

    monkeypatch.setattr(lq.LinearFlexibleLqer, "gated_min_m", 1)
    logits = []
    ids = torch.randint(0, 320, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)
    for fuse in (True, False):
        model = quantize_model(_tiny_llama(), {"linear": MXINT_Q}, {"linear": {"rank": 16}}, fuse_mlp=fuse)
        load_low_rank_dict(model, _ab_dict(model, 16))
        model = model.to(DEV).half()
        with torch.no_grad():
            logits.append(model(input_ids=ids).logits.float().cpu())
        down = model.model.layers[0].mlp.down_proj
        assert any(k[0] == "gated" for k in down._fw_cache) == fuse  # the fused entry really ran
    assert torch.isfinite(logits[0]).all()
    err = float((logits[0] - logits[1]).norm() / logits[1].norm())
    print(f"rel-L2 of the logits, fused against unfused: {err:.3e}")
    assert err <= 3e-3

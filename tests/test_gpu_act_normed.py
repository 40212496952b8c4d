"""RMSNorm inside the activation side of the Linears behind it (lqer_amd/csrc/act_normed.hip: lqer_quantize_act_xa_normed,
lqer_linear_forward_normed, LinearFlexibleLqer.forward_normed, a SharedActivation round armed with the raw hidden state,
quantize_model(fuse_norm=True)) against the four-line formula of include/lqer_hip.h evaluated on the CPU in torch fp32:
    S = sum h^2,  rstd = 1 / sqrt(S / K + eps),  n = round_dt(h * rstd),  x = round_dt(w * n)
h is integers / 16, so every square is a multiple of 2^-8 and S (< 2^24 such units for K <= 8192) is exact in fp32 in ANY order: the
formula gives the kernel's x bit for bit, no element exempted.  Then the oracle's quantizers: the activation image bit for bit, x_q A
inside the summation-order envelope and bit-stable, the forward at the parity gate; a q/k/v-like group; a tiny Llama.
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
EPS = 1e-5
F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 1e-3, BF16: 5e-3}  # tests/test_gpu_parity.py, per output dtype (1e-3 for fp16)


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return __import__("lqer_amd")


def _inputs(M, K, dt, seed):
    """(h, w) in dt: h = integers in [-40, 40] / 16 with three outlier channels at +-30, an all-zero block and (from two rows on: a
    lone row of zeros would leave nothing to check) an all-zero last row; w = 1 + 0.1 randn."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randint(-40, 41, (M, K), generator=gen).float() / 16
    for c in (7, 100, K - 3):
        h[:, c] = 30.0 * (2 * torch.randint(0, 2, (M,), generator=gen).float() - 1)
    h[0, 16:32] = 0.0
    if M > 1:
        h[M - 1] = 0.0
    return h.to(dt), (1 + 0.1 * torch.randn(K, generator=gen)).to(dt)


def _x_ref(h, w, eps=EPS):
    """The header's four lines in torch fp32 on the CPU (division and square root correctly rounded)."""
    S = (h.float() ** 2).sum(-1, keepdim=True)
    assert torch.equal(S.double(), (h.double() ** 2).sum(-1, keepdim=True))  # exact: any order gives these bits
    rstd = 1.0 / (S / h.shape[-1] + eps).sqrt()
    n = (h.float() * rstd).to(h.dtype)
    return (w.float() * n.float()).to(h.dtype)


CASES = [
    # M, K, rank, dtype, x width
    (1, 512, 32, F16, 8),      # below a row group, one slab, seven waves with no slab but in the reduction
    (8, 640, 16, F16, 8),      # one full group, a part-filled second slab
    (13, 4608, 96, BF16, 8),   # a ragged group, wave 0 keeps two slabs in registers, six rank tiles
    (24, 8192, 128, F16, 4),   # the largest K, eight tiles, a narrow format
    (13, 640, 0, BF16, 8),     # rank 0: the image alone
    (24, 4608, 48, BF16, 4),   # three rank tiles
]


@pytest.mark.parametrize("M,K,r,dt,xw", CASES)
def test_normed_activation_side_and_forward(lq, M, K, r, dt, xw):
    from bench import MXINT_Q, _bfp, make_weights
    from lqer_amd import _lib, ops

    qc = dict(MXINT_Q, x_quantizer=_bfp(xw, [1, 16], True))
    h, w = _inputs(M, K, dt, seed=M + K + r)
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
    a_img = mod._normed_a_image() if r else None
    assert desc.rank == r and (not r or a_img is not None)
    hd, wd = h.to(DEV), w.to(DEV)
    Kp, Mp, rp = L.lqer_padded_k(K), L.lqer_padded_m(M), L.lqer_padded_r(r) if r else 0
    xaq_off = (Mp * Kp * 2 + 255) // 256 * 256
    (a_t, b_t), st = (a_img.data_ptr(), p["b_t"].data_ptr()) if r else (None, None), torch.cuda.current_stream().cuda_stream
    lead = (C.byref(desc), hd.data_ptr(), wd.data_ptr(), EPS, ops.dtype_code(hd), M, hd.stride(0))

    def read(ws):
        torch.cuda.synchronize()
        img = ws[: Mp * Kp * 2].view(torch.bfloat16).view(Mp, Kp)[:M].clone()
        return img, ws[xaq_off: xaq_off + Mp * rp * 2].view(torch.bfloat16).view(Mp, rp)[:M].float().cpu() if r else None

    ws = torch.full((ops.linear_sizes(desc, M).workspace,), 0x5A, dtype=torch.uint8, device=DEV)
    y = torch.empty(M, N, dtype=dt, device=DEV)
    _lib.check(L.lqer_linear_forward_normed(*lead, p["w"].data_ptr(), a_t, b_t, -2, p.get("b_limbs", 0), None, y.data_ptr(), N, ws.data_ptr(),
                                            ws.numel(), st), "linear_forward_normed")
    img, xa = read(ws)
    ws2 = torch.full_like(ws, 0xA5)
    _lib.check(L.lqer_quantize_act_xa_normed(*lead, a_t, -2, ws2.data_ptr(), ws2.data_ptr() + xaq_off if r else None, st), "quantize_act_xa_normed")
    img2, xa2 = read(ws2)
    # (1) the image: the oracle's quantizer applied to x_ref, bit for bit (|x| <= 1e-8 flushed in images), zeros in the padded k
    x = _x_ref(h, w).float()
    ref = O.get_quantizer(qc["x_quantizer"])(x)
    assert torch.equal(img[:, :K].float().cpu(), torch.where(x.abs() <= 1e-8, torch.zeros_like(ref), ref))
    assert Kp == K or float(img[:, K:].float().abs().max()) == 0.0
    # (2) x_q A inside the envelope of the exact sum of exact products; the split entry on another workspace: identical bits
    assert torch.equal(img.view(torch.int16), img2.view(torch.int16))
    if r:
        s64 = img[:, :K].double().cpu().numpy() @ A.to(dt).double().numpy()
        assert envelope_check(s64, xa[:, :r].numpy(), 16, xw - 1, max(16.0, math.sqrt(K))) == 0
        assert torch.equal(xa, xa2)
    # (3) the forward against the oracle's on x_ref
    c = lambda t: t.to(dt).float()
    want = O.lqer_linear_forward(x, c(W), None, c(A) if r else None, c(B) if r else None, qc)
    err = float((y.float().cpu() - want).norm() / want.norm())
    print(f"rel-L2 of y against the oracle: {err:.3e}")
    assert err <= TOL[dt]


def test_group_round_from_the_raw_hidden_state(lq, monkeypatch):
    """Three rank-32 Linears over one K = 640 in a SharedActivation (padded rank 96), 13 tokens: every member's output of the round armed
    with (h, w, eps) against its own output on the torch-normalised tensor."""
    from bench import MXINT_Q, make_weights

    monkeypatch.setattr(lq.LinearFlexibleLqer, "normed_min_m", 1)
    M, K = 13, 640
    mods = []
    for i in range(3):
        W, A, B = make_weights(torch.Generator().manual_seed(i), K, N, 32)
        m = lq.LinearFlexibleLqer(K, N, bias=False, q_config=MXINT_Q, l_config={"rank": 32})
        m.load_state_dict({"weight": W, "A": A, "B": B})
        mods.append(m.to(DEV).half())
    g = lq.linear.SharedActivation(mods)
    h, w = (t.to(DEV) for t in _inputs(M, K, F16, seed=3))
    xn = lq.LinearFlexibleLqer.rms_norm_torch(h, w, EPS)
    want = [m(xn).float() for m in mods]
    assert g.enabled and g.normed_rounds == 0 and g.normed_serves(h)
    g.arm_normed(h, w, EPS)
    got = [m(h).float() for m in mods]
    assert g.normed_rounds == 1  # the normed entry really ran, once for the three members
    for a, b in zip(got, want):
        err = float((a - b).norm() / b.norm())
        print(f"rel-L2 of a member against itself on the torch norm: {err:.3e}")
        assert err <= TOL[F16]


def test_tiny_llama_with_and_without_the_fused_norm(lq, monkeypatch):
    """fuse_norm=True, fuse_mlp=True against fuse_norm=False on the fp16 model of tests/test_model_swap.py: the two routes differ by
    torch's rsqrt against 1 / sqrt - that file's tolerance for two fp16 routes of one model (3e-3).  48 tokens: both fused entries are
    switched on below the token counts from which the modules take them by default."""
    from bench import MXINT_Q
    from lqer_amd.models import load_low_rank_dict, quantize_model
    from test_model_swap import _ab_dict, _tiny_llama

    monkeypatch.setattr(lq.LinearFlexibleLqer, "gated_min_m", 1)
    monkeypatch.setattr(lq.LinearFlexibleLqer, "normed_min_m", 1)
    logits = []
    ids = torch.randint(0, 320, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)
    for fuse in (True, False):
        model = quantize_model(_tiny_llama(), {"linear": MXINT_Q}, {"linear": {"rank": 16}}, fuse_mlp=True, fuse_norm=fuse)
        load_low_rank_dict(model, _ab_dict(model, 16))
        model = model.to(DEV).half()
        with torch.no_grad():
            logits.append(model(input_ids=ids).logits.float().cpu())
        layer = model.model.layers[1]
        assert [layer.self_attn.q_proj._group.normed_rounds, layer.mlp.gate_proj._group.normed_rounds] == [int(fuse)] * 2
    assert torch.isfinite(logits[0]).all()
    err = float((logits[0] - logits[1]).norm() / logits[1].norm())
    print(f"rel-L2 of the logits, fused norm against torch norm: {err:.3e}")
    assert err <= 3e-3

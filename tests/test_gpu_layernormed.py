"""The fused LayerNorm (lqer_amd/csrc/act_normed.hip, NORM_LAYER) against the rule of include/lqer_hip.h evaluated on the CPU in torch fp32:
    mean = sum h / K,  d = h - mean,  rstd = 1 / sqrt(sum d^2 / K + eps),  x = round_dt((d * rstd) * w + b)
h is built so that both sums are exact in fp32 in ANY order (rows of integers / 16 that sum to zero, plus an integer mean): the rule gives
the kernel's x bit for bit, no element exempted.  Then the oracle's quantizers, as tests/test_gpu_act_normed.py.  -m gpu."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _envelope import envelope_check  # noqa: E402
from oracle import lqer_oracle as O  # noqa: E402
from test_gpu_act_normed import BF16, DEV, EPS, F16, N, TOL, lq  # noqa: E402,F401  (that file's constants and module fixture)


def _inputs(M, K, dt, seed):
    """(h, w, b) in dt: the first half of the columns integers / 16 with two outlier channels and a zero block, the second half its negated
    permutation, + an integer mean per row; a zero last row (M > 1) and the constant 1.5 before it (M > 2)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randint(-40, 41, (M, K // 2), generator=gen).float() / 16
    for c in (7, K // 2 - 3):
        a[:, c] = 30.0 * (2 * torch.randint(0, 2, (M,), generator=gen).float() - 1)
    a[:, 16:32] = 0.0
    h = torch.cat([a, -a[:, torch.randperm(K // 2, generator=gen)]], 1) + torch.randint(-2, 3, (M, 1), generator=gen).float()
    h[M - 1 if M > 1 else M:] = 0.0
    h[M - 2 if M > 2 else M: M - 1] = 1.5
    return h.to(dt), (1 + 0.1 * torch.randn(K, generator=gen)).to(dt), (0.1 * torch.randn(K, generator=gen)).to(dt)


def _x_ref(h, w, b, eps=EPS):
    """The header's rule, one fp32 rounding per operation; S1, mean and S2 are asserted exact against fp64."""
    K, h64 = h.shape[-1], h.double()
    S1 = h.float().sum(-1, keepdim=True)
    mean = S1 / K
    d = h.float() - mean
    S2 = (d * d).sum(-1, keepdim=True)
    assert torch.equal(S1.double(), h64.sum(-1, keepdim=True)) and torch.equal(mean.double(), h64.mean(-1, keepdim=True))
    assert torch.equal(S2.double(), ((h64 - mean.double()) ** 2).sum(-1, keepdim=True))
    return ((d * (1.0 / (S2 / K + eps).sqrt())) * w.float() + b.float()).to(h.dtype)


def _modules(lq, n, K, r, qc, dt):
    from bench import make_weights

    out = []
    for i in range(n):
        W, A, B = make_weights(torch.Generator().manual_seed(K + r + i), K, N, max(r, 1))
        mod = (lq.LinearFlexibleLqer(K, N, bias=False, q_config=qc, l_config={"rank": r}) if r else
               lq.LinearFlexible(K, N, bias=False, q_config=dict(qc, name="flexible")))
        mod.load_state_dict({"weight": W, "A": A, "B": B} if r else {"weight": W})
        out.append((mod.to(DEV).to(dt), W, A, B))
    return out


@pytest.fixture
def from_one_token(lq, monkeypatch):
    for cls, name in ((lq.LinearFlexibleLqer, "gated_min_m"), (lq.LinearFlexibleLqer, "layer_normed_min_m"),
                      (lq.linear.SharedActivation, "layer_normed_min_m")):
        monkeypatch.setattr(cls, name, 1)


@pytest.mark.parametrize("M,K,r,dt,xw", [
    (1, 512, 32, F16, 8),      # one row, one slab, seven waves with no slab in both reductions
    (13, 640, 16, F16, 8),     # a ragged row group and a part-filled second slab: the lanes past K
    (13, 4608, 96, BF16, 8),   # wave 0 keeps two slabs in registers, six rank tiles
    (24, 8192, 128, F16, 4),   # the largest K, eight tiles, a narrow format
    (13, 640, 0, BF16, 8),     # rank 0: the image alone
])
def test_layernormed_activation_side_and_forward(lq, M, K, r, dt, xw):
    from bench import MXINT_Q, _bfp
    from lqer_amd import _lib, ops

    qc = dict(MXINT_Q, x_quantizer=_bfp(xw, [1, 16], True))
    h, w, b = _inputs(M, K, dt, seed=M + K + r)
    (mod, W, A, B), = _modules(lq, 1, K, r, qc, dt)
    mod._pack()
    p, desc, L = mod._packed, mod._desc(), _lib.lib()
    a_img = mod._normed_a_image() if r else None
    assert desc.rank == r and (not r or a_img is not None)
    hd, wd, bd = h.to(DEV), w.to(DEV), b.to(DEV)
    Kp, Mp, rp = L.lqer_padded_k(K), L.lqer_padded_m(M), L.lqer_padded_r(r) if r else 0
    xaq_off = (Mp * Kp * 2 + 255) // 256 * 256
    (a_t, b_t), st = (a_img.data_ptr(), p["b_t"].data_ptr()) if r else (None, None), torch.cuda.current_stream().cuda_stream
    lead = (C.byref(desc), hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), EPS, ops.dtype_code(hd), M, hd.stride(0))

    def read(ws):
        torch.cuda.synchronize()
        img = ws[: Mp * Kp * 2].view(torch.bfloat16).view(Mp, Kp)[:M].clone()
        return img, ws[xaq_off: xaq_off + Mp * rp * 2].view(torch.bfloat16).view(Mp, rp)[:M].float().cpu() if r else None

    ws = torch.full((ops.linear_sizes(desc, M).workspace,), 0x5A, dtype=torch.uint8, device=DEV)
    ws2, y = torch.full_like(ws, 0xA5), torch.empty(M, N, dtype=dt, device=DEV)
    _lib.check(L.lqer_linear_forward_layernormed(*lead, p["w"].data_ptr(), a_t, b_t, -2, p.get("b_limbs", 0), None, y.data_ptr(), N,
                                                 ws.data_ptr(), ws.numel(), st), "linear_forward_layernormed")
    _lib.check(L.lqer_quantize_act_xa_layernormed(*lead, a_t, -2, ws2.data_ptr(), ws2.data_ptr() + xaq_off if r else None, st),
               "quantize_act_xa_layernormed")
    (img, xa), (img2, xa2) = read(ws), read(ws2)
    # (0) the rule: the zero row and the constant row give b; against nn.LayerNorm in fp64 at most one step of dt (bit patterns as ordinals)
    xr = _x_ref(h, w, b)
    assert all(torch.equal(xr[M - i], b) for i in (1, 2) if M > i)
    x64 = F.layer_norm(h.double(), (K,), w.double(), b.double(), EPS).to(dt)
    o = [torch.where(t < 0, -(t & 0x7FFF), t) for t in (t.view(torch.int16).int() for t in (xr, x64))]
    print(f"x against fp64 LayerNorm rounded to {dt}: at most {int((o[0] - o[1]).abs().max())} step(s)")
    assert int((o[0] - o[1]).abs().max()) <= 1
    # (1) the image: the oracle's quantizer applied to x_ref, bit for bit (|x| <= 1e-8 flushed in images), zeros in the padded k
    x = xr.float()
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


@pytest.mark.parametrize("members", [3, 1])
def test_round_from_the_raw_hidden_state(lq, from_one_token, members):
    """A q/k/v-like group of three and a lone Linear (fc1) armed with (h, w, b, eps), against their own outputs on F.layer_norm(h)."""
    from bench import MXINT_Q

    M, K = 13, 640
    mods = [m for m, *_ in _modules(lq, members, K, 32, MXINT_Q, F16)]
    h, w, b = (t.to(DEV) for t in _inputs(M, K, F16, seed=3))
    armed = lq.linear.SharedActivation(mods) if members > 1 else mods[0]
    assert members == 1 or (armed.enabled and armed.normed_serves(h, layer_norm=True))
    rounds = lambda: armed.normed_rounds if members > 1 else armed.layer_normed_rounds
    want = [m(F.layer_norm(h, (K,), w, b, EPS)).float() for m in mods]
    assert rounds() == 0
    armed.arm_layer_normed(h, w, b, EPS)
    got = [m(h).float() for m in mods]
    assert rounds() == 1  # the fused entry really ran, once
    for a, c in zip(got, want):
        print(f"rel-L2 of a module against itself on the torch norm: {float((a - c).norm() / c.norm()):.3e}")
        assert float((a - c).norm() / c.norm()) <= TOL[F16]


def test_tiny_opt_with_and_without_the_fused_layernorm(lq, from_one_token):
    """Two fp16 routes of the OPT of tests/test_model_swap.py at that file's tolerance (3e-3); 48 tokens, so the thresholds are lowered."""
    from bench import OPT_Q
    from lqer_amd.models import load_low_rank_dict, quantize_model
    from test_model_swap import _ab_dict, _tiny_opt

    logits = []
    ids = torch.randint(0, 200, (2, 24), generator=torch.Generator().manual_seed(5)).to(DEV)
    for fuse in (True, False):
        model = quantize_model(_tiny_opt(), {"linear": OPT_Q}, {"linear": {"rank": 16}}, fuse_mlp=True, fuse_layernorm=fuse)
        load_low_rank_dict(model, _ab_dict(model, 16))
        model = model.to(DEV).half()
        with torch.no_grad():
            logits.append(model(input_ids=ids).logits.float().cpu())
        layer = model.model.decoder.layers[1]
        assert [layer.self_attn.q_proj._group.normed_rounds, layer.fc1.layer_normed_rounds] == [int(fuse)] * 2
    err = float((logits[0] - logits[1]).norm() / logits[1].norm())
    print(f"rel-L2 of the logits, fused LayerNorm against torch LayerNorm: {err:.3e}")
    assert torch.isfinite(logits[0]).all() and err <= 3e-3

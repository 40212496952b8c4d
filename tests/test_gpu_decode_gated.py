"""The decode step behind a gated MLP (csrc/decode1_kernel.h's GATE instantiations, lqer_linear_decode_gated): y on (g, u) is BIT-equal to
y of the existing one-launch entry handed h_ref - tests/test_gpu_act_gated.py's inputs zero g wherever fp32 cannot be asked for silu's bits."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import lqer_oracle as O  # noqa: E402
from test_gpu_act_gated import BF16, DEV, F16, N, TOL, _h_ref, _inputs, lq  # noqa: E402,F401


def _mod(lq, K, r, dt, bias=False):
    from bench import MXINT_Q, make_weights

    W, A, B = make_weights(torch.Generator().manual_seed(K + r), K, N, r)
    m = lq.LinearFlexibleLqer(K, N, bias=bias, q_config=MXINT_Q, l_config={"rank": r})
    m.load_state_dict(dict({"weight": W, "A": A, "B": B}, **({"bias": torch.randn(N, generator=torch.Generator().manual_seed(K))} if bias else {})))
    return m.to(DEV).to(dt)


def _fused(mod, g, u, act):
    mod._pack()
    y = mod._forward_decode_gated(g, u, {"silu": 0, "relu": 1}[act])  # (_lib.ACT_SILU, _lib.ACT_RELU)
    assert y is not None  # (None: the one-launch entry refused)
    return y


@pytest.mark.parametrize("M,K,r,dt,operands,bias,tune", [
    (1, 512, 32, F16, "separate", False, 0),     # two producers, most lanes idle
    (8, 640, 16, F16, "halves", False, 0),       # full rows, a short last producer, strided rows of one [M, 2K] tensor
    (5, 4608, 48, BF16, "separate", False, 0),   # three rank tiles, bf16 rounding of s and h
    (6, 11008, 32, F16, "separate", False, 0),   # the down projection's K: one workgroup per CU, more image blocks than one pass of 512 threads
    (4, 640, 16, BF16, "relu", True, 0),         # OPT's fc2 form: relu, up = None, with bias
    (8, 640, 16, F16, "separate", False, 1),     # LQER_TUNE_DECODE_NO_POLL: the consumers' own produce() forming h
])
def test_bit_equal_to_the_x_entry_on_h_ref(lq, M, K, r, dt, operands, bias, tune):
    from lqer_amd import _lib

    act = "relu" if operands == "relu" else "silu"
    g, u = _inputs(M, K, dt, seed=M + K + r)
    u = None if operands == "relu" else u
    mod = _mod(lq, K, r, dt, bias)
    mod.tuning = _lib.TUNE_DECODE_NO_POLL if tune else 0
    assert _lib.lib().lqer_decode_partials(C.byref(mod._desc(plain=True)), M) == 1
    # (from the formats alone; `want`'s route also needs decode1_lds_bytes(M, Kp, 1) <= 150 KiB: 141328 B at M = 6, K = 11008)
    pitch = -(-_lib.lib().lqer_padded_k(K) * 2 // 256) * 256
    assert max(M * pitch, 32 * 1024) + 8192 + 1024 + 16 <= 150 * 1024
    want = mod(_h_ref(g, u, act).to(DEV))  # lqer_linear_forward: the one-launch decode route
    gd, ud = g.to(DEV), None if u is None else u.to(DEV)
    if operands == "halves":
        gd, ud = torch.cat([g, u], dim=1).to(DEV).split(K, dim=1)
    got = _fused(mod, gd, ud, act)
    torch.cuda.synchronize()
    assert mod.decode_gated_rounds == 1 and torch.equal(got, want)


def test_general_inputs_at_the_parity_gate_and_bit_stable(lq):
    """y against the oracle's forward on h evaluated in fp64 and rounded to the dtype, at the parity gate; three calls: the same bits."""
    from bench import MXINT_Q, make_weights

    M, K, r, dt = 5, 1088, 32, F16
    gen = torch.Generator().manual_seed(9)
    g, u = (4 * torch.randn(M, K, generator=gen)).to(dt), torch.randn(M, K, generator=gen)
    u[:, (7, 100, K - 3)] *= 30.0
    h = ((g.double() / (1 + torch.exp(-g.double()))).to(dt).double() * u.to(dt).double()).to(dt)
    mod = _mod(lq, K, r, dt)
    ys = [_fused(mod, g.to(DEV), u.to(dt).to(DEV), "silu").clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    c = lambda t: t.to(dt).float()
    W, A, B = make_weights(torch.Generator().manual_seed(K + r), K, N, r)  # (the module's own)
    want = O.lqer_linear_forward(h.float(), c(W), None, c(A), c(B), MXINT_Q)
    err = float((ys[0].float().cpu() - want).norm() / want.norm())
    print(f"rel-L2 of y against the oracle on the fp64 h: {err:.3e}")
    assert err <= TOL[dt]


def test_under_graph_capture_one_kernel_node(lq, monkeypatch):
    """forward_gated at M = 4 with the entry switched on: ONE kernel node, and the replays follow new contents of g and u."""
    from lqer_amd.graph import GraphedCallable

    monkeypatch.setattr(lq.LinearFlexibleLqer, "decode_gated", True)
    monkeypatch.setattr(lq.LinearFlexibleLqer, "decode_gated_max_m", 8)  # (the default threshold lies below these 4 tokens)
    M, K = 4, 1024
    mod = _mod(lq, K, 32, F16)
    gus = [_inputs(M, K, F16, seed) for seed in (11, 12)]
    want = [mod(_h_ref(g, u, "silu").to(DEV)) for g, u in gus]
    gs, us = gus[0][0].to(DEV), gus[0][1].to(DEV)
    gc = GraphedCallable(lambda g, u: mod.forward_gated(g, u), gs, us, warmup=1, keep_graph=True)
    assert mod.decode_gated_rounds == 2 and gc.kernel_nodes() == 1  # the warm-up and the capture; ONE kernel node captured
    for i in (1, 0, 1):
        gs.copy_(gus[i][0]), us.copy_(gus[i][1])
        out = gc(gs, us).clone()
        torch.cuda.synchronize()
        assert torch.equal(out, want[i]), i


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_tiny_models_decode_step_with_and_without_the_fused_mlp(lq, family, monkeypatch):
    """M = 2 x 3 through tests/test_model_swap.py's tiny models: fuse_mlp against torch's activation at that file's 3e-3, one new round."""
    import test_model_swap as T
    from bench import MXINT_Q, OPT_Q
    from lqer_amd.models import load_low_rank_dict, quantize_model

    monkeypatch.setattr(lq.LinearFlexibleLqer, "decode_gated", True)
    monkeypatch.setattr(lq.LinearFlexibleLqer, "decode_gated_max_m", 8)
    ids = torch.randint(0, 200, (2, 3), generator=torch.Generator().manual_seed(5)).to(DEV)  # (the tiny OPT has 200 tokens, the Llama 320)
    make, qc = (T._tiny_llama, MXINT_Q) if family == "llama" else (T._tiny_opt, OPT_Q)
    logits = []
    for fuse in (True, False):
        model = quantize_model(make(), {"linear": qc}, {"linear": {"rank": 16}}, fuse_mlp=fuse)
        load_low_rank_dict(model, T._ab_dict(model, 16))
        model = model.to(DEV).half()
        with torch.no_grad():
            logits.append(model(input_ids=ids).logits.float().cpu())
        layer = (model.model if family == "llama" else model.model.decoder).layers[1]
        assert (layer.mlp.down_proj if family == "llama" else layer.fc2).decode_gated_rounds == int(fuse)
    err = float((logits[0] - logits[1]).norm() / logits[1].norm())
    print(f"rel-L2 of the logits, fused MLP against the torch activation: {err:.3e}")
    assert torch.isfinite(logits[0]).all() and err <= 3e-3

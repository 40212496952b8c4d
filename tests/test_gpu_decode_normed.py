"""The decode step behind a norm (csrc/decode1.hip's NORM instantiations): y of the new entry on (h, w[, b], eps) is BIT-equal to y of the
existing one-launch entry handed x_ref, the header's rule evaluated on the CPU - the inputs of tests/test_gpu_act_normed.py /
test_gpu_layernormed.py make S, S1 and S2 exact in fp32 in any order, so x_ref has the kernel's x bits.  python -m pytest tests -m gpu"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_act_normed as R  # noqa: E402
import test_gpu_layernormed as LNT  # noqa: E402
from oracle import lqer_oracle as O  # noqa: E402
from test_gpu_act_normed import BF16, DEV, EPS, F16, N, TOL, lq  # noqa: E402,F401

NORMS = ["rms", "layer"]


def _case(norm, M, K, dt, seed):  # (h, w, b or None, x_ref) on the CPU
    if norm == "rms":
        h, w = R._inputs(M, K, dt, seed)
        return h, w, None, R._x_ref(h, w)
    h, w, b = LNT._inputs(M, K, dt, seed)
    return h, w, b, LNT._x_ref(h, w, b)


def _mods(lq, Ns, K, r, dt):
    from bench import MXINT_Q, make_weights

    mods = []
    for i, n in enumerate(Ns):
        W, A, B = make_weights(torch.Generator().manual_seed(K + r + i), K, n, r)
        m = lq.LinearFlexibleLqer(K, n, bias=False, q_config=MXINT_Q, l_config={"rank": r})
        m.load_state_dict({"weight": W, "A": A, "B": B})
        mods.append(m.to(DEV).to(dt))
    return mods


def _fused(mod, h, w, b):
    mod._pack()
    y = mod._forward_decode_normed(h.to(DEV), w.to(DEV), EPS, None if b is None else b.to(DEV))
    assert y is not None  # (None: the one-launch entry refused)
    return y


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("M,K,r,dt,tune", [
    (1, 512, 32, F16, 0),    # one slab, seven waves empty in both reductions, two producers
    (8, 640, 16, F16, 0),    # full rows, a part-filled second slab, a short last producer
    (5, 4608, 48, BF16, 0),  # wave 0 owns two slabs, three rank tiles
    (6, 8192, 64, F16, 0),   # the largest K; more image blocks than one pass of 512 threads x 4; one workgroup per CU
    (8, 640, 16, F16, 1),    # LQER_TUNE_DECODE_NO_POLL: the consumers' own produce() with the norm
])
def test_one_linear_bit_equal_to_the_x_entry_on_x_ref(lq, norm, M, K, r, dt, tune):
    from lqer_amd import _lib

    h, w, b, x = _case(norm, M, K, dt, seed=M + K + r)
    (mod,) = _mods(lq, (N,), K, r, dt)
    mod.tuning = _lib.TUNE_DECODE_NO_POLL if tune else 0
    assert _lib.lib().lqer_decode_partials(C.byref(mod._desc(plain=True)), M) == 1
    want = mod(x.to(DEV))  # lqer_linear_forward: the one-launch decode route
    got = _fused(mod, h, w, b)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("norm", NORMS)
def test_group_bit_equal_and_under_graph_capture(lq, norm, monkeypatch):
    """Ns (512, 256, 384) over K = 1024, rank 32 each (96 concatenated rank columns: two chunks in produce()), M = 4: the armed round is
    the group's ONE launch (one round counted for the three members), and a captured round's replays follow new contents of h."""
    from lqer_amd.graph import GraphedCallable

    monkeypatch.setattr(lq.linear.SharedActivation, "decode_normed", True)
    monkeypatch.setattr(lq.linear.SharedActivation, "decode_layer_normed", True)
    M, K = 4, 1024
    mods = _mods(lq, (512, 256, 384), K, 32, F16)
    g = lq.linear.SharedActivation(mods)
    _, w, b, _ = _case(norm, M, K, F16, 11)
    hs = [_case(norm, M, K, F16, seed)[0] for seed in (11, 12)]
    xs = [R._x_ref(h, w) if b is None else LNT._x_ref(h, w, b) for h in hs]
    want = [[m(x.to(DEV)) for m in mods] for x in xs]  # lqer_linear_forward_group on x_ref
    wd, bd = w.to(DEV), None if b is None else b.to(DEV)

    def armed(h):
        assert g.normed_serves(h, layer_norm=bd is not None)
        g.arm_normed(h, wd, EPS) if bd is None else g.arm_layer_normed(h, wd, bd, EPS)
        return [m(h) for m in mods]

    got = armed(hs[0].to(DEV))
    assert g.normed_rounds == 1 and all(torch.equal(a, c) for a, c in zip(got, want[0]))
    gc = GraphedCallable(armed, hs[0].to(DEV), warmup=1, keep_graph=True)
    assert g.normed_rounds == 3 and gc.kernel_nodes() == 1  # the warm-up and the capture: one group launch each, ONE kernel node captured
    for i in (1, 0, 1):
        out = [t.clone() for t in gc(hs[i].to(DEV))]
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(out, want[i])), i


@pytest.mark.parametrize("norm", NORMS)
def test_general_inputs_at_the_parity_gate_and_bit_stable(lq, norm):
    """randn h with a row of zeros and a row with a large mean: y against the oracle's forward on the norm evaluated in fp64 and rounded
    to the dtype, at the project's parity gate; three calls give the same bits."""
    from bench import MXINT_Q, make_weights

    M, K, r, dt = 5, 1088, 32, F16
    gen = torch.Generator().manual_seed(9)
    h = torch.randn(M, K, generator=gen)
    h[1], h[3] = 0.0, h[3] + 40.0
    h = h.to(dt)
    w, b = (1 + 0.1 * torch.randn(K, generator=gen)).to(dt), (0.1 * torch.randn(K, generator=gen)).to(dt)
    h64 = h.double()
    if norm == "rms":
        b = None
        x = (w.double() * (h64 / (h64.pow(2).mean(-1, keepdim=True) + EPS).sqrt()).to(dt).double()).to(dt)
    else:
        d = h64 - h64.mean(-1, keepdim=True)
        x = (d / (d.pow(2).mean(-1, keepdim=True) + EPS).sqrt() * w.double() + b.double()).to(dt)
    (mod,) = _mods(lq, (N,), K, r, dt)
    ys = [_fused(mod, h, w, b).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    c = lambda t: t.to(dt).float()
    W, A, B = make_weights(torch.Generator().manual_seed(K + r), K, N, r)  # (the module's own: _mods' first seed)
    want = O.lqer_linear_forward(x.float(), c(W), None, c(A), c(B), MXINT_Q)
    err = float((ys[0].float().cpu() - want).norm() / want.norm())
    print(f"rel-L2 of y against the oracle on the fp64 norm: {err:.3e}")
    assert err <= TOL[dt]


@pytest.mark.parametrize("family", ["llama", "opt"])
def test_tiny_models_decode_step_with_and_without_the_fused_norm(lq, family, monkeypatch):
    """2 x 3 tokens (M = 6) through the tiny models of tests/test_model_swap.py, the decode entries switched on: fused against torch norm
    at that file's tolerance for two fp16 routes (3e-3), one armed round per group (and per fc1)."""
    import test_model_swap as T
    from bench import MXINT_Q, OPT_Q
    from lqer_amd.models import load_low_rank_dict, quantize_model

    for cls in (lq.linear.SharedActivation, lq.LinearFlexibleLqer):
        monkeypatch.setattr(cls, "decode_normed", True)
        monkeypatch.setattr(cls, "decode_layer_normed", True)
    ids = torch.randint(0, 200, (2, 3), generator=torch.Generator().manual_seed(5)).to(DEV)  # (the tiny OPT has 200 tokens, the Llama 320)
    make, qc, flag = (T._tiny_llama, MXINT_Q, "fuse_norm") if family == "llama" else (T._tiny_opt, OPT_Q, "fuse_layernorm")
    logits = []
    for fuse in (True, False):
        model = quantize_model(make(), {"linear": qc}, {"linear": {"rank": 16}}, **{flag: fuse})
        load_low_rank_dict(model, T._ab_dict(model, 16))
        model = model.to(DEV).half()
        with torch.no_grad():
            logits.append(model(input_ids=ids).logits.float().cpu())
        layer = (model.model if family == "llama" else model.model.decoder).layers[1]
        second = layer.mlp.gate_proj._group.normed_rounds if family == "llama" else layer.fc1.layer_normed_rounds
        assert [layer.self_attn.q_proj._group.normed_rounds, second] == [int(fuse)] * 2
    err = float((logits[0] - logits[1]).norm() / logits[1].norm())
    print(f"rel-L2 of the logits, fused norm against torch norm: {err:.3e}")
    assert torch.isfinite(logits[0]).all() and err <= 3e-3

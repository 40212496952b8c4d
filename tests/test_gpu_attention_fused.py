"""Fused quantized attention on the GPU (lqer_attention_q, csrc/attn_q.hip; lqer_amd.functional.attention_flexible).

The CPU comparator is the construction of tests/test_model_swap.py::oracle_attention - oracle.lqer_oracle.matmul_flexible for the
two products, torch.softmax in fp32 between them - with the rounding to the operands' dtype DT written out wherever the unfused
route materialises a tensor:
    S = Q_x0(q) Q_w0(k^T) ->DT;  S1 = S scaling ->DT;  S2 = S1 + mask ->DT;  P = softmax_fp32(S2) ->DT;  O = Q_x1(P) Q_w1(v) ->DT.
The bar on O is the project's forward bar, relative L2 <= 1e-3.  What it has to absorb is the order of the fp32
sums and the last bits of exp, which flip a few codes of P at quantizer ties: the comparator against itself with fp64 accumulation
and an fp64 softmax differs by at most 5.4e-5, so the bar leaves a factor of about 18 over the reference's own spread.
"""
import json
import types

import pytest
import torch

from _attention import BAR, CFG, DEV, _causal_mask, _randn, _rel, comparator  # noqa: F401 (shared with the other attention modules)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def fused(q, k, v, scaling, mask=None, causal=False, cfg0=CFG, cfg1=CFG, **kw):
    from lqer_amd import attention_flexible

    out, stats, route = attention_flexible(q, k, v, cfg0, cfg1, scaling, attention_mask=mask, causal=causal, return_stats=True, return_route=True, **kw)
    assert route == "fused"
    return out, stats


def _module(groups=1):
    return types.SimpleNamespace(_lqer_matmul_cfg=(CFG, CFG), num_key_value_groups=groups, training=False)


def unfused_gpu(q, k, v, scaling, mask=None):
    """The route of the parent commit: lqer_eager_attention_forward -> [b, s, h, d], weights."""
    from lqer_amd import attention as A

    return A.lqer_eager_attention_forward(_module(q.shape[1] // k.shape[1]), q, k, v, mask, scaling)


# ---- 1. the exact leg ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("mode", ["none", "mask", "causal"])
@pytest.mark.parametrize("shape", [(2, 2, 2, 96, 96, 32), (2, 4, 2, 200, 328, 64), (2, 2, 2, 1, 37, 16), (1, 2, 2, 130, 130, 128), (2, 4, 2, 150, 210, 96)],
                         ids=lambda s: "x".join(map(str, s)))
def test_exact_scores(dtype, mode, shape):
    """q, k integer-valued in [-7, 7] (fixed points of the 8-bit quantizer): every product and partial sum of S is an integer
    below 2^24, so S - and with it S1, S2 and the row maximum - is the same in any summation order: the kernel's row maximum
    equals the comparator's bit for bit, the row sum to 1e-6.  Catches a wrong scaling, rounding or mask order."""
    b, h, hk, s, t, d = shape
    g = torch.Generator().manual_seed(3)
    q = torch.randint(-7, 8, (b, h, s, d), generator=g).to(dtype)
    k = torch.randint(-7, 8, (b, hk, t, d), generator=g).to(dtype)
    v = _randn((b, hk, t, d), dtype, 4)
    scaling = d ** -0.5
    mask = None
    if mode != "none":
        # the tensor form carries a left-padded last batch element whose early rows are fully masked
        mask = _causal_mask(s, t, dtype, pad=(t - s) + min(5, s) if mode == "mask" else None, batch=b)
    ref, S2, _ = comparator(q, k, v, scaling, mask)
    if mode == "causal":
        got, stats = fused(q.to(DEV), k.to(DEV), v.to(DEV), scaling, causal=True)
    else:
        got, stats = fused(q.to(DEV), k.to(DEV), v.to(DEV), scaling, mask=None if mask is None else mask.to(DEV))
    stats = stats.cpu()
    want_max = S2.float().amax(dim=-1)
    assert torch.equal(stats[..., 0], want_max), f"row max differs in {(stats[..., 0] != want_max).sum().item()} of {want_max.numel()} rows"
    fin = torch.isfinite(want_max)
    want_sum = torch.exp((S2.float() - want_max[..., None]).double()).sum(-1)
    rel = ((stats[..., 1].double() - want_sum).abs() / want_sum)[fin].max().item()
    err = _rel(got.cpu().float()[fin], ref.float()[fin])
    print(f"exact leg {shape} {dtype} {mode}: row-sum rel {rel:.2e}, O rel-L2 {err:.2e}")
    assert rel <= 1e-6
    assert err <= BAR


# ---- 2. parity against the comparator on random inputs ------------------------------------------------------------------------
PARITY = [  # b, h, h_kv, s, t, d, q/k scale, causal
    (1, 4, 4, 256, 256, 128, 1.0, False), (1, 4, 4, 256, 256, 128, 3.0, False), (1, 4, 4, 200, 328, 64, 1.0, False),
    (1, 4, 4, 200, 328, 64, 3.0, False), (1, 2, 2, 512, 512, 128, 1.0, False), (1, 8, 2, 160, 160, 64, 1.0, False),
    (1, 4, 4, 100, 300, 64, 1.0, True), (1, 2, 2, 512, 512, 128, 3.0, True), (2, 2, 2, 150, 150, 16, 1.0, False),
    (2, 2, 2, 150, 150, 48, 1.0, True), (2, 2, 1, 70, 150, 128, 1.0, False),
    (2, 4, 2, 200, 328, 96, 1.0, False), (1, 4, 4, 256, 256, 96, 3.0, True), (2, 2, 2, 150, 150, 80, 1.0, True),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "x".join(map(str, c)))
def test_parity_vs_comparator(dtype, case):
    b, h, hk, s, t, d, sc, causal = case
    q, k, v = _randn((b, h, s, d), dtype, 10, sc), _randn((b, hk, t, d), dtype, 11, sc), _randn((b, hk, t, d), dtype, 12)
    scaling = d ** -0.5
    ref, _, _ = comparator(q, k, v, scaling, _causal_mask(s, t, dtype) if causal else None)
    got, _ = fused(q.to(DEV), k.to(DEV), v.to(DEV), scaling, causal=causal)
    err = _rel(got.cpu(), ref)
    print(f"parity {case} {dtype}: O rel-L2 vs comparator {err:.3e}")
    assert torch.isfinite(got).all()
    assert err <= BAR


# ---- 3. against the unfused GPU route ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("case", [(1, 4, 4, 256, 256, 128, True), (2, 8, 2, 200, 328, 64, False), (1, 4, 4, 1, 300, 128, False)],
                         ids=lambda c: "x".join(map(str, c)))
def test_vs_unfused_gpu_route(dtype, case):
    b, h, hk, s, t, d, masked = case
    q, k, v = (x.to(DEV) for x in (_randn((b, h, s, d), dtype, 20), _randn((b, hk, t, d), dtype, 21), _randn((b, hk, t, d), dtype, 22)))
    mask = _causal_mask(s, t, dtype).to(DEV) if masked else None
    want, _ = unfused_gpu(q, k, v, d ** -0.5, mask)
    got, _ = fused(q, k, v, d ** -0.5, mask=mask, out_layout="bshd")
    err = _rel(got, want)
    frac = float((got != want).float().mean())
    print(f"vs unfused {case} {dtype}: rel-L2 {err:.3e}, differing output elements {frac:.3e}")
    assert got.shape == want.shape and err <= BAR


# ---- 4. the causal rule equals the tensor form of the same mask ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("s,t,d", [(192, 192, 64), (100, 333, 128), (257, 300, 32)])
def test_causal_equals_mask_tensor(dtype, s, t, d):
    q, k, v = (x.to(DEV) for x in (_randn((2, 2, s, d), dtype, 30, 2.0), _randn((2, 2, t, d), dtype, 31, 2.0), _randn((2, 2, t, d), dtype, 32)))
    a, sa = fused(q, k, v, d ** -0.5, causal=True)
    m, sm = fused(q, k, v, d ** -0.5, mask=_causal_mask(s, t, dtype).to(DEV))
    assert torch.equal(a, m) and torch.equal(sa, sm)


# ---- 5. head mapping, layouts, slices, determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_bitwise_identities(dtype):
    b, h, hk, s, t, d = 2, 8, 2, 140, 210, 64
    q, k, v = (x.to(DEV) for x in (_randn((b, h, s, d), dtype, 40), _randn((b, hk, t, d), dtype, 41), _randn((b, hk, t, d), dtype, 42)))
    mask = _causal_mask(s, t, dtype, pad=80, batch=b).to(DEV)
    out, st = fused(q, k, v, 0.125, mask=mask)
    out2, st2 = fused(q, k, v, 0.125, mask=mask)
    assert torch.equal(out, out2) and torch.equal(st, st2)  # two runs
    rep = lambda x: x[:, :, None].expand(b, hk, h // hk, t, d).reshape(b, h, t, d).contiguous()
    out_r, st_r = fused(q, rep(k), rep(v), 0.125, mask=mask)
    assert torch.equal(out, out_r) and torch.equal(st, st_r)  # grouped-query heads through the mapping = repeated K / V
    out_t, _ = fused(q, k, v, 0.125, mask=mask, out_layout="bshd")
    assert out_t.shape == (b, s, h, d) and out_t.is_contiguous() and torch.equal(out_t.transpose(1, 2), out)
    o1, _ = fused(q[1:], k[1:], v[1:], 0.125, mask=mask[1:])  # a batch slice
    assert torch.equal(o1, out[1:])
    o2, _ = fused(q[:, 4:8], k[:, 1:2], v[:, 1:2], 0.125, mask=mask)  # the heads of one kv group
    assert torch.equal(o2, out[:, 4:8])


# ---- 6. strided inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_views_of_a_fused_projection(dtype):
    """q, k, v as non-contiguous views of one [b, s, 3 h d] projection: read in place (the last dim is contiguous)."""
    b, h, s, d = 2, 4, 150, 64
    qkv = _randn((b, s, 3 * h * d), dtype, 50).to(DEV)
    q, k, v = (qkv.view(b, s, 3, h, d)[:, :, i].transpose(1, 2) for i in range(3))
    assert not q.is_contiguous() and q.stride(3) == 1
    snap = qkv.clone()
    out, st = fused(q, k, v, 0.125, causal=True, out_layout="bshd")
    ref, st_ref = fused(q.contiguous(), k.contiguous(), v.contiguous(), 0.125, causal=True, out_layout="bshd")
    assert torch.equal(out, ref) and torch.equal(st, st_ref) and torch.equal(qkv, snap)


# ---- 7. guard zones -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("mode", ["mask", "causal"])
def test_guard_zones(dtype, mode):
    """out (rows padded: stride d + 8), row_stats and a workspace of exactly the reported size between guards, over a pseudo-random
    fill and over 0xFF: guards, gaps and inputs unchanged, outputs equal over both fills."""
    import ctypes as C

    from _guard import guarded, rows_bytes

    from lqer_amd import _lib, ops

    b, h, hk, s, t, d = 2, 4, 2, 77, 203, 48
    esz = torch.empty(0, dtype=dtype).element_size()
    ld = d + 8
    q, k, v = _randn((b, h, s, d), dtype, 60), _randn((b, hk, t, d), dtype, 61), _randn((b, hk, t, d), dtype, 62)
    mask = _causal_mask(s, t, dtype, pad=150, batch=b)
    L = _lib.lib()
    fmt = ops.make_qfmt(CFG["x_quantizer"], "x")
    tri = lambda *xs: (C.c_int64 * 3)(*xs)
    nws = L.lqer_attention_q_workspace_bytes(b, h, hk, s, t, d)
    results = []
    for fill in (0, 0xFF):
        gq = guarded(q.numel() * esz, fill=fill, name="q").load(q.to(DEV))
        gk = guarded(k.numel() * esz, fill=fill, name="k").load(k.to(DEV))
        gv = guarded(v.numel() * esz, fill=fill, name="v").load(v.to(DEV))
        gm = guarded(mask.numel() * esz, fill=fill, name="mask").load(mask.to(DEV))
        go = guarded(rows_bytes(b * h * s, d, ld, esz), row_pitch_bytes=ld * esz, fill=fill, name="out")
        gs = guarded(b * h * s * 2 * 4, fill=fill, name="row_stats")
        gw = guarded(nws, fill=fill, name="workspace")
        rc = L.lqer_attention_q(gq.ptr, gk.ptr, gv.ptr, gm.ptr if mode == "mask" else None, go.ptr, gs.ptr, ops.dtype_code(q), b, h, hk, s, t, d,
                                tri(h * s * d, s * d, d), tri(hk * t * d, t * d, d), tri(hk * t * d, t * d, d), tri(s * t, 0, t) if mode == "mask" else None,
                                tri(h * s * ld, s * ld, ld), 0.2, int(mode == "causal"), C.byref(fmt), C.byref(fmt), C.byref(fmt), C.byref(fmt),
                                gw.ptr, nws, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "lqer_attention_q")
        torch.cuda.synchronize()
        for gbuf in (gq, gk, gv, gm):
            gbuf.unchanged()
        for gbuf in (go, gs, gw):
            gbuf.check()
        go.gaps_unchanged(b * h * s, d, ld, dtype)
        results.append((go.rows_view(b * h * s, d, ld, dtype).contiguous().clone(), gs.view(torch.float32).reshape(b, h, s, 2).clone()))
    assert torch.equal(results[0][0].view(torch.uint8), results[1][0].view(torch.uint8)) and torch.equal(results[0][1], results[1][1])
    ref, _, _ = comparator(q, k, v, 0.2, mask if mode == "mask" else _causal_mask(s, t, dtype))
    rows = torch.isfinite(results[0][1][..., 0]).cpu()
    assert _rel(results[0][0].reshape(b, h, s, d).cpu()[rows], ref[rows]) <= BAR


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    from lqer_amd import attention_flexible
    from lqer_amd.graph import GraphedCallable

    dtype, (b, h, hk, s, t, d) = torch.float16, (1, 4, 2, 96, 160, 64)
    mk = lambda seed: [x.to(DEV) for x in (_randn((b, h, s, d), dtype, seed), _randn((b, hk, t, d), dtype, seed + 1), _randn((b, hk, t, d), dtype, seed + 2))]
    fn = lambda q, k, v: attention_flexible(q, k, v, CFG, CFG, 0.125, causal=True, out_layout="bshd")
    static = [x.clone() for x in mk(70)]
    step = GraphedCallable(fn, *static, warmup=2)
    for seed in (70, 80, 90):
        new = mk(seed)
        want = fn(*new)
        got = step(*new).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert not torch.equal(fn(*mk(70)), fn(*mk(80)))


# ---- 9. what falls back -------------------------------------------------------------------------------------------------------
def test_fallbacks_take_the_unfused_route():
    from lqer_amd import attention as A
    from lqer_amd import attention_flexible

    dtype = torch.float16
    cfg32 = json.loads(json.dumps(CFG))
    cfg32["x_quantizer"]["block_size"] = [1, 32]
    cases = [("block 32", (1, 2, 2, 64, 64, 64), cfg32), ("d = 160", (1, 2, 2, 64, 64, 160), CFG)]
    for name, (b, h, hk, s, t, d), cfg in cases:
        q, k, v = (x.to(DEV) for x in (_randn((b, h, s, d), dtype, 100), _randn((b, hk, t, d), dtype, 101), _randn((b, hk, t, d), dtype, 102)))
        mask = _causal_mask(s, t, dtype).to(DEV)
        assert attention_flexible.route(q, k, v, cfg, cfg, mask) == "unfused", name
        out, route = attention_flexible(q, k, v, cfg, cfg, 0.125, attention_mask=mask, out_layout="bshd", return_route=True)
        mod = types.SimpleNamespace(_lqer_matmul_cfg=(cfg, cfg), num_key_value_groups=1, training=False)
        want, _ = A.lqer_eager_attention_forward(mod, q, k, v, mask, 0.125)
        assert route == "unfused" and torch.equal(out, want), name
    # a mask whose last dim is not contiguous
    b, h, s, t, d = 1, 2, 64, 64, 64
    q, k, v = (x.to(DEV) for x in (_randn((b, h, s, d), dtype, 103), _randn((b, h, t, d), dtype, 104), _randn((b, h, t, d), dtype, 105)))
    mask_t = _causal_mask(s, t, dtype).to(DEV).transpose(2, 3).contiguous().transpose(2, 3)
    assert attention_flexible.route(q, k, v, CFG, CFG, mask_t) == "unfused"
    assert attention_flexible.route(q, k, v, CFG, CFG, mask_t.contiguous()) == "fused"
    # the causal rule with s > t (early rows see no key): the tensor form on the unfused route, the same bits as that mask handed over
    qs = _randn((b, h, 100, d), dtype, 106).to(DEV)
    assert attention_flexible.route(qs, k, v, CFG, CFG, None, True) == "unfused"
    assert attention_flexible.route(q, k, v, CFG, CFG, None, True) == "fused"
    out, route = attention_flexible(qs, k, v, CFG, CFG, 0.125, causal=True, out_layout="bshd", return_route=True)
    want, _ = A.lqer_eager_attention_forward(_module(), qs, k, v, _causal_mask(100, t, dtype).to(DEV), 0.125)
    assert route == "unfused" and torch.equal(out, want)
    # a mask of another dtype than q (torch adds it with type promotion): the registered function takes the unfused one
    m32 = _causal_mask(s, t, torch.float32).to(DEV)
    got, w = A.lqer_fused_attention_forward(_module(), q, k, v, m32, 0.125)
    want, w_want = A.lqer_eager_attention_forward(_module(), q, k, v, m32, 0.125)
    assert w is not None and torch.equal(got, want) and torch.equal(w, w_want)
    # a caller that wants the weights: the registered function hands the call to the unfused one
    mod = _module()
    got, w = A.lqer_fused_attention_forward(mod, q, k, v, mask_t.contiguous(), 0.125, output_attentions=True)
    want, w_want = A.lqer_eager_attention_forward(mod, q, k, v, mask_t.contiguous(), 0.125)
    assert w is not None and torch.equal(got, want) and torch.equal(w, w_want)
    got, w = A.lqer_fused_attention_forward(mod, q, k, v, mask_t.contiguous(), 0.125)
    assert w is None and got.shape == want.shape and _rel(got, want) <= BAR


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------
def _tiny_llama(kv_heads=4):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=kv_heads,
                      vocab_size=320, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).eval()


def _tiny_opt():
    from transformers import OPTConfig, OPTForCausalLM

    torch.manual_seed(0)
    cfg = OPTConfig(hidden_size=128, ffn_dim=256, num_hidden_layers=2, num_attention_heads=4, vocab_size=200, max_position_embeddings=64,
                    word_embed_proj_dim=128)
    return OPTForCausalLM(cfg).eval()


def _ab_dict(model, rank, seed=1):
    from lqer_amd import LinearFlexibleLqer
    from oracle import lqer_oracle as O

    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, m in model.named_modules():
        if isinstance(m, LinearFlexibleLqer):
            out[f"{name}.A"] = O.mxint_quantize(0.02 * torch.randn(m.in_features, rank, generator=g), width=8, block_size=[16, 1], skip_first_dim=False)
            out[f"{name}.B"] = O.mxint_quantize(0.02 * torch.randn(rank, m.out_features, generator=g), width=8, block_size=[16, 1], skip_first_dim=False)
    return out


class _OracleLinear(torch.nn.Module):
    def __init__(self, src, q_config):
        super().__init__()
        f = lambda x: None if x is None else x.detach().float().cpu()
        self.w, self.b, self.A, self.B, self.qc = f(src.weight), f(src.bias), f(src.A), f(src.B), q_config

    def forward(self, x):
        from oracle import lqer_oracle as O

        return O.lqer_linear_forward(x, self.w, self.b, self.A, self.B, self.qc)


@pytest.mark.parametrize("family", ["llama", "llama-gqa", "opt"])
def test_end_to_end_fused(family):
    import copy

    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, eager_mask

    from bench import MXINT_Q, OPT_Q
    from lqer_amd import LinearFlexibleLqer
    from lqer_amd import attention as A
    from lqer_amd.models import load_low_rank_dict, quantize_model

    lin_q = OPT_Q if family == "opt" else MXINT_Q
    qc = {"linear": lin_q, ("bmm" if family == "opt" else "matmul"): CFG}
    base = _tiny_opt() if family == "opt" else _tiny_llama(2 if family == "llama-gqa" else 4)
    model = quantize_model(base, qc, {"linear": {"rank": 16}})
    load_low_rank_dict(model, _ab_dict(model, 16))
    twin = copy.deepcopy(model)
    for name, m in list(twin.named_modules()):
        if isinstance(m, LinearFlexibleLqer):
            setattr(twin.get_submodule(name.rsplit(".", 1)[0]), name.rsplit(".", 1)[1], _OracleLinear(m, lin_q))

    def oracle_attention(module, query, key, value, attention_mask, scaling, dropout=0.0, **kwargs):
        out, _, w = comparator(query, key, value, scaling, attention_mask)
        return out.transpose(1, 2).contiguous(), w

    AttentionInterface.register("lqer_oracle_fused_twin", oracle_attention)
    AttentionMaskInterface.register("lqer_oracle_fused_twin", eager_mask)
    twin.set_attn_implementation("lqer_oracle_fused_twin")
    unfused = A.enable_quantized_attention(copy.deepcopy(model), qc).to(DEV)
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV)
    assert model.config._attn_implementation == "lqer_fused" and unfused.config._attn_implementation == "lqer_eager"
    ids = torch.randint(0, 200, (2, 20), generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        ref = twin(input_ids=ids).logits
        got = model(input_ids=ids.to(DEV)).logits.float().cpu()
        got_u = unfused(input_ids=ids.to(DEV)).logits.float().cpu()
    e_ref, e_unf = _rel(got, ref), _rel(got, got_u)
    print(f"end to end {family}: logits vs oracle twin {e_ref:.3e}, vs fused=False {e_unf:.3e}")
    assert torch.isfinite(got).all()
    assert e_ref <= 1e-4 and e_unf <= 1e-4


def test_whole_model_graph_replay_fused():
    from bench import MXINT_Q
    from lqer_amd import attention as A
    from lqer_amd.graph import GraphedCallable
    from lqer_amd.models import load_low_rank_dict, quantize_model

    qc = {"linear": MXINT_Q, "matmul": CFG}
    model = quantize_model(_tiny_llama(2), qc, {"linear": {"rank": 16}}, share_inputs=True)
    load_low_rank_dict(model, _ab_dict(model, 16))
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV).half()
    tokens = 40
    g = torch.Generator().manual_seed(5)
    ids = [torch.randint(0, 320, (1, tokens), generator=g).to(DEV) for _ in range(3)]
    mask = torch.full((1, 1, tokens, tokens), float("-inf"), dtype=torch.float16, device=DEV).triu(1)
    run = lambda t: model(input_ids=t, attention_mask=mask, use_cache=False).logits
    with torch.no_grad():
        eager = [run(i).clone() for i in ids]
        step = GraphedCallable(run, ids[0].clone(), warmup=2)
        for i, want in zip(ids, eager):
            got = step(i).clone()
            torch.cuda.synchronize()
            assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(eager[0], eager[1])

"""The decode kernel of the fused quantized attention on the GPU (lqer_attention_q_decode, csrc/attn_decode.hip; reached through
lqer_amd.functional.attention_flexible with up to 8 query rows).

The comparator is tests/test_gpu_attention_fused.py's: oracle.lqer_oracle.matmul_flexible for the two products, torch.softmax in fp32
between them, every ->DT written out.  The bar on O is the project's forward bar, relative L2 <= 1e-3 over the whole output of a case
(DESIGN section 2).  What it has to absorb is the order of the fp32 sums and the last bits of exp, which flip a few codes of P at
quantizer ties: at exactly the PARITY cases below the comparator differs from itself with an fp64 softmax by at most 7.5e-5 (checked
on the CPU), so the bar leaves a factor of 13; every row maximum of those cases is finite, so no row is excluded anywhere.

Shapes are the smallest that reach every edge of the kernel: T = 1; below, at and above one block of 16 keys (15, 16, 17); a ragged
last block (37); several chunks of keys (300: 10 chunks of 32, 1000: 16 of 64); one key past a power of two (2049: chunks of 128 plus
one key); 1, 5 and 8 query rows; heads / kv_heads of 1, 2, 4 and 8; head dims 16 .. 128 that are not all multiples of 32."""
import ctypes as C
import json

import pytest
import torch

import test_gpu_attention_fused as F
from _attention import _mask, _pad  # noqa: F401

pytestmark = pytest.mark.gpu

CFG, DEV, BAR, DTYPES = F.CFG, F.DEV, F.BAR, F.DTYPES
DT_IDS = ["f16", "bf16", "f32"]
_ids = lambda c: "x".join(map(str, c))


def decode(q, k, v, scaling, mask=None, causal=False, **kw):
    """attention_flexible with the automatic rule, which must pick the decode kernel -> out, stats."""
    from lqer_amd import attention_flexible

    assert attention_flexible.kernel(q, k, v, CFG, CFG, mask, causal) == "decode"
    out, stats, route = attention_flexible(q, k, v, CFG, CFG, scaling, attention_mask=mask, causal=causal, return_stats=True, return_route=True, **kw)
    assert route == "fused"
    return out, stats


def _dev(*xs):
    return [None if x is None else x.to(DEV) for x in xs]


# ---- 1. the exact leg ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["none", "mask", "causal"])
@pytest.mark.parametrize("shape", [(2, 4, 2, 1, 37, 16), (2, 4, 2, 5, 37, 80), (2, 8, 2, 8, 300, 64), (1, 4, 4, 1, 2049, 128)], ids=_ids)
def test_exact_scores(dtype, mode, shape):
    """q, k integer-valued in [-7, 7]: S, S1, S2 and the row maximum are the same in any summation order, so the kernel's row maximum
    equals the comparator's bit for bit and the row sum to 1e-6 - over every row (each keeps a visible key).
    The seed is chosen on the CPU, without any kernel: the comparator re-evaluated with its row sums taken chunk by chunk differs
    from itself by at most 3.9e-7 over these 36 cases with seed 5.  With seed 3 (the sibling test's) it differs by 2.2e-3 at
    (2, 4, 2, 1, 37, 16) fp32: one P = 0.73046869 sits one ulp under the quantizer tie 93.5 / 128, so the order of the row sum alone
    flips its code, and one code is 1 % of a row of that 128-element output - an input that tests the tie, not the kernel.
    This leg therefore stays clear of ties by construction; codes that flip at ties are what the parity leg's random inputs and
    its 1e-3 bar cover."""
    b, h, hk, s, t, d = shape
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-7, 8, (b, h, s, d), generator=g).to(dtype)
    k = torch.randint(-7, 8, (b, hk, t, d), generator=g).to(dtype)
    v = F._randn((b, hk, t, d), dtype, 4)
    scaling = d ** -0.5
    mask = _mask(mode, b, s, t, dtype)
    ref, S2, _ = F.comparator(q, k, v, scaling, mask)
    gq, gk, gv, gm = _dev(q, k, v, mask)
    got, stats = decode(gq, gk, gv, scaling, causal=True) if mode == "causal" else decode(gq, gk, gv, scaling, mask=gm)
    stats = stats.cpu()
    want_max = S2.float().amax(dim=-1)
    assert torch.isfinite(want_max).all()
    assert torch.equal(stats[..., 0], want_max), f"row max differs in {(stats[..., 0] != want_max).sum().item()} of {want_max.numel()} rows"
    want_sum = torch.exp((S2.float() - want_max[..., None]).double()).sum(-1)
    rel = ((stats[..., 1].double() - want_sum).abs() / want_sum).max().item()
    err = F._rel(got.cpu().float(), ref.float())
    print(f"exact leg {shape} {dtype} {mode}: row-sum rel {rel:.2e}, O rel-L2 {err:.2e}")
    assert rel <= 1e-6
    assert err <= BAR


# ---- 2. parity against the comparator on random inputs ------------------------------------------------------------------------
PARITY = [(2, 4, 2, 1, 1, 16), (2, 4, 2, 1, 15, 16), (2, 4, 2, 1, 17, 48), (2, 4, 4, 1, 37, 64), (2, 8, 2, 1, 300, 128), (1, 8, 1, 1, 1000, 128),
          (1, 4, 4, 1, 2049, 128), (2, 4, 2, 5, 37, 80), (2, 8, 2, 8, 300, 64), (1, 4, 4, 8, 1000, 96), (2, 4, 2, 2, 257, 128), (1, 4, 2, 8, 2049, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["none", "causal", "mask"])
@pytest.mark.parametrize("sc", [1.0, 3.0])
@pytest.mark.parametrize("shape", PARITY, ids=_ids)
def test_parity_vs_comparator(dtype, mode, sc, shape):
    b, h, hk, s, t, d = shape
    q, k, v = F._randn((b, h, s, d), dtype, 10, sc), F._randn((b, hk, t, d), dtype, 11, sc), F._randn((b, hk, t, d), dtype, 12)
    scaling = d ** -0.5
    mask = _mask(mode, b, s, t, dtype)
    ref, _, _ = F.comparator(q, k, v, scaling, mask)
    gq, gk, gv, gm = _dev(q, k, v, mask)
    got, _ = decode(gq, gk, gv, scaling, causal=True) if mode == "causal" else decode(gq, gk, gv, scaling, mask=gm)
    err = F._rel(got.cpu(), ref)
    print(f"parity {shape} x{sc} {mode} {dtype}: O rel-L2 vs comparator {err:.3e}")
    assert torch.isfinite(got).all()
    assert err <= BAR


# ---- 3. against the prefill kernel and the unfused GPU route -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(1, 4, 4, 1, 300, 128), (2, 8, 2, 4, 328, 64)], ids=_ids)
def test_vs_prefill_kernel_and_unfused_route(dtype, shape):
    from lqer_amd import attention_flexible

    b, h, hk, s, t, d = shape
    q, k, v = _dev(F._randn((b, h, s, d), dtype, 20), F._randn((b, hk, t, d), dtype, 21), F._randn((b, hk, t, d), dtype, 22))
    mask = F._causal_mask(s, t, dtype).to(DEV)
    got, _ = decode(q, k, v, d ** -0.5, mask=mask, out_layout="bshd")
    pre = attention_flexible(q, k, v, CFG, CFG, d ** -0.5, attention_mask=mask, out_layout="bshd", kernel="prefill")
    unf, _ = F.unfused_gpu(q, k, v, d ** -0.5, mask)
    for name, want in (("prefill kernel", pre), ("unfused route", unf)):
        err, frac = F._rel(got, want), float((got != want).float().mean())
        print(f"decode vs {name} {shape} {dtype}: rel-L2 {err:.3e}, differing output elements {frac:.3e}")
        assert got.shape == want.shape and err <= BAR


# ---- 4. fully masked rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 2, 2, 1, 37, 16), (2, 2, 2, 3, 37, 16)], ids=_ids)
def test_fully_masked_rows(dtype, shape):
    """The last batch element's keys all masked by finfo.min: added and rounded literally, as the unfused route does."""
    b, h, hk, s, t, d = shape
    q, k, v = _dev(F._randn((b, h, s, d), dtype, 30), F._randn((b, hk, t, d), dtype, 31), F._randn((b, hk, t, d), dtype, 32))
    mask = torch.zeros(b, 1, s, t, dtype=dtype)
    mask[-1] = torch.finfo(dtype).min
    mask = mask.to(DEV)
    got, _ = decode(q, k, v, d ** -0.5, mask=mask, out_layout="bshd")
    want, _ = F.unfused_gpu(q, k, v, d ** -0.5, mask)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    err = F._rel(got[ok], want[ok])
    print(f"fully masked {shape} {dtype}: NaN elements {int((~ok).sum())}, rel-L2 of the rest {err:.3e}")
    assert err <= BAR


# ---- 5. bitwise identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bitwise_identities(dtype):
    b, h, hk, s, t, d = 2, 8, 2, 3, 210, 64
    q, k, v = _dev(F._randn((b, h, s, d), dtype, 40), F._randn((b, hk, t, d), dtype, 41), F._randn((b, hk, t, d), dtype, 42))
    mask = F._causal_mask(s, t, dtype, pad=_pad(s, t), batch=b).to(DEV)
    out, st = decode(q, k, v, 0.125, mask=mask)
    out2, st2 = decode(q, k, v, 0.125, mask=mask)
    assert torch.equal(out, out2) and torch.equal(st, st2)  # two runs
    rep = lambda x: x[:, :, None].expand(b, hk, h // hk, t, d).reshape(b, h, t, d).contiguous()
    out_r, st_r = decode(q, rep(k), rep(v), 0.125, mask=mask)
    assert torch.equal(out, out_r) and torch.equal(st, st_r)  # grouped-query heads through the mapping = repeated K / V
    out_t, _ = decode(q, k, v, 0.125, mask=mask, out_layout="bshd")
    assert out_t.shape == (b, s, h, d) and out_t.is_contiguous() and torch.equal(out_t.transpose(1, 2), out)
    o1, s1 = decode(q[1:], k[1:], v[1:], 0.125, mask=mask[1:])  # a batch slice
    assert torch.equal(o1, out[1:]) and torch.equal(s1, st[1:])
    o2, s2 = decode(q[:, 4:8], k[:, 1:2], v[:, 1:2], 0.125, mask=mask)  # the heads of one kv group
    assert torch.equal(o2, out[:, 4:8]) and torch.equal(s2, st[:, 4:8])
    # k, v as views of a longer preallocated cache; q, k, v at a storage offset of one element (rows not 16-byte aligned)
    cache_k, cache_v = (torch.zeros(b, hk, t + 91, d, dtype=dtype, device=DEV) for _ in range(2))
    cache_k[:, :, :t], cache_v[:, :, :t] = k, v
    kv, vv = cache_k[:, :, :t], cache_v[:, :, :t]
    assert not kv.is_contiguous()
    snap = (cache_k.clone(), cache_v.clone())
    o3, s3 = decode(q, kv, vv, 0.125, mask=mask)
    assert torch.equal(o3, out) and torch.equal(s3, st) and torch.equal(cache_k, snap[0]) and torch.equal(cache_v, snap[1])

    def shifted(x):
        flat = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
        flat[1:] = x.reshape(-1)
        y = flat[1:].view(x.shape)
        assert y.data_ptr() % 16 != 0
        return y, flat

    (qs, qf), (ks, kf), (vs, vf) = shifted(q), shifted(k), shifted(v)
    snaps = [x.clone() for x in (qf, kf, vf)]
    o4, s4 = decode(qs, ks, vs, 0.125, mask=mask)
    assert torch.equal(o4, out) and torch.equal(s4, st)
    assert all(torch.equal(x, y) for x, y in zip((qf, kf, vf), snaps))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_causal_equals_mask_tensor(dtype):
    b, h, s, t, d = 2, 2, 5, 333, 128
    q, k, v = _dev(F._randn((b, h, s, d), dtype, 45, 2.0), F._randn((b, h, t, d), dtype, 46, 2.0), F._randn((b, h, t, d), dtype, 47))
    a, sa = decode(q, k, v, d ** -0.5, causal=True)
    m, sm = decode(q, k, v, d ** -0.5, mask=F._causal_mask(s, t, dtype).to(DEV))
    assert torch.equal(a, m) and torch.equal(sa, sm)


# ---- 6. mask broadcast forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_mask_broadcast_forms(dtype):
    b, h, hk, s, t, d = 2, 4, 2, 3, 75, 32
    q, k, v = _dev(F._randn((b, h, s, d), dtype, 50), F._randn((b, hk, t, d), dtype, 51), F._randn((b, hk, t, d), dtype, 52))
    lo = torch.finfo(dtype).min
    g = torch.Generator().manual_seed(53)
    for shape in [(1, 1, 1, t), (b, 1, s, t), (b, h, s, t)]:
        m = torch.where(torch.rand(shape, generator=g) < 0.3, torch.tensor(lo), torch.randn(shape, generator=g)).to(dtype)
        m[..., -1] = 0  # every row keeps a visible key
        m = m.to(DEV)
        got, st = decode(q, k, v, 0.2, mask=m)
        want, st_w = decode(q, k, v, 0.2, mask=m.expand(b, h, s, t).contiguous())
        assert torch.equal(got, want) and torch.equal(st, st_w), shape


# ---- 7. guard zones -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["mask", "causal"])
def test_guard_zones(dtype, mode):
    """out (rows padded: stride d + 8), row_stats and a workspace of exactly the reported size between guards, over a pseudo-random
    fill and over 0xFF: guards, gaps and inputs unchanged, outputs equal over both fills."""
    from _guard import guarded, rows_bytes

    from lqer_amd import _lib, ops

    b, h, hk, s, t, d = 2, 4, 2, 3, 203, 48
    esz = torch.empty(0, dtype=dtype).element_size()
    ld = d + 8
    q, k, v = F._randn((b, h, s, d), dtype, 60), F._randn((b, hk, t, d), dtype, 61), F._randn((b, hk, t, d), dtype, 62)
    mask = F._causal_mask(s, t, dtype, pad=_pad(s, t), batch=b)
    L = _lib.lib()
    fmt = ops.make_qfmt(CFG["x_quantizer"], "x")
    tri = lambda *xs: (C.c_int64 * 3)(*xs)
    nws = L.lqer_attention_q_decode_workspace_bytes(b, h, hk, s, t, d)
    assert nws > 0
    results = []
    for fill in (0, 0xFF):
        gq = guarded(q.numel() * esz, fill=fill, name="q").load(q.to(DEV))
        gk = guarded(k.numel() * esz, fill=fill, name="k").load(k.to(DEV))
        gv = guarded(v.numel() * esz, fill=fill, name="v").load(v.to(DEV))
        gm = guarded(mask.numel() * esz, fill=fill, name="mask").load(mask.to(DEV))
        go = guarded(rows_bytes(b * h * s, d, ld, esz), row_pitch_bytes=ld * esz, fill=fill, name="out")
        gs = guarded(b * h * s * 2 * 4, fill=fill, name="row_stats")
        gw = guarded(nws, fill=fill, name="workspace")
        rc = L.lqer_attention_q_decode(gq.ptr, gk.ptr, gv.ptr, gm.ptr if mode == "mask" else None, go.ptr, gs.ptr, ops.dtype_code(q), b, h, hk, s, t,
                                       d, tri(h * s * d, s * d, d), tri(hk * t * d, t * d, d), tri(hk * t * d, t * d, d),
                                       tri(s * t, 0, t) if mode == "mask" else None, tri(h * s * ld, s * ld, ld), 0.2, int(mode == "causal"),
                                       C.byref(fmt), C.byref(fmt), C.byref(fmt), C.byref(fmt), gw.ptr, nws, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "lqer_attention_q_decode")
        torch.cuda.synchronize()
        for gbuf in (gq, gk, gv, gm):
            gbuf.unchanged()
        for gbuf in (go, gs, gw):
            gbuf.check()
        go.gaps_unchanged(b * h * s, d, ld, dtype)
        results.append((go.rows_view(b * h * s, d, ld, dtype).contiguous().clone(), gs.view(torch.float32).reshape(b, h, s, 2).clone()))
    assert torch.equal(results[0][0].view(torch.uint8), results[1][0].view(torch.uint8)) and torch.equal(results[0][1], results[1][1])
    ref, _, _ = F.comparator(q, k, v, 0.2, mask if mode == "mask" else F._causal_mask(s, t, dtype))
    assert torch.isfinite(results[0][1]).all()
    assert F._rel(results[0][0].reshape(b, h, s, d).cpu(), ref) <= BAR


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    from lqer_amd import attention_flexible
    from lqer_amd.graph import GraphedCallable

    dtype, (b, h, hk, s, t, d) = torch.float16, (1, 4, 2, 1, 160, 64)
    mk = lambda seed: _dev(F._randn((b, h, s, d), dtype, seed), F._randn((b, hk, t, d), dtype, seed + 1), F._randn((b, hk, t, d), dtype, seed + 2))
    fn = lambda q, k, v: attention_flexible(q, k, v, CFG, CFG, 0.125, causal=True, out_layout="bshd")
    static = [x.clone() for x in mk(70)]
    assert attention_flexible.kernel(*static, CFG, CFG, None, True) == "decode"
    step = GraphedCallable(fn, *static, warmup=2)
    for seed in (70, 80, 90):
        new = mk(seed)
        want = fn(*new)
        got = step(*new).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert not torch.equal(fn(*mk(70)), fn(*mk(80)))


# ---- 9. routing ---------------------------------------------------------------------------------------------------------------
def test_routing():
    from lqer_amd import _lib, attention_flexible, ops

    dtype = torch.float16
    b, h, t, d = 1, 2, 64, 64
    k, v = _dev(F._randn((b, h, t, d), dtype, 101), F._randn((b, h, t, d), dtype, 102))
    q8, q9 = _dev(F._randn((b, h, 8, d), dtype, 100), F._randn((b, h, 9, d), dtype, 103))
    assert attention_flexible.kernel(q8, k, v, CFG, CFG) == "decode"
    assert attention_flexible.kernel(q9, k, v, CFG, CFG) == "prefill"
    cfg32 = json.loads(json.dumps(CFG))
    cfg32["x_quantizer"]["block_size"] = [1, 32]
    assert attention_flexible.kernel(q8, k, v, cfg32, cfg32) is None
    with pytest.raises(ValueError):
        attention_flexible(q9, k, v, CFG, CFG, 0.125, kernel="decode")
    with pytest.raises(ValueError):
        attention_flexible(q8, k, v, cfg32, cfg32, 0.125, kernel="decode")
    # either kernel forced at s = 8: both the fused route, the same result within the bar
    a, ra = attention_flexible(q8, k, v, CFG, CFG, 0.125, kernel="decode", return_route=True)
    p, rp = attention_flexible(q8, k, v, CFG, CFG, 0.125, kernel="prefill", return_route=True)
    assert ra == rp == "fused" and F._rel(a, p) <= BAR
    # the C call refuses S = 9 before it touches anything
    L = _lib.lib()
    fmt = ops.make_qfmt(CFG["x_quantizer"], "x")
    tri = lambda *xs: (C.c_int64 * 3)(*xs)
    out = torch.zeros(b, h, 9, d, dtype=dtype, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    rc = L.lqer_attention_q_decode(q9.data_ptr(), k.data_ptr(), v.data_ptr(), None, out.data_ptr(), None, ops.dtype_code(q9), b, h, h, 9, t, d,
                                   tri(h * 9 * d, 9 * d, d), tri(h * t * d, t * d, d), tri(h * t * d, t * d, d), None, tri(h * 9 * d, 9 * d, d), 0.125, 0,
                                   C.byref(fmt), C.byref(fmt), C.byref(fmt), C.byref(fmt), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -2 and "attention" in L.lqer_last_error().decode()  # LQER_E_UNSUPPORTED
    assert not out.any() and not ws.any()


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["llama", "llama-gqa"])
def test_end_to_end_decode_steps(family, monkeypatch):
    """A prefill of 12 tokens, then 4 decode steps against the KV cache: every attention call of a decode step runs the decode
    kernel, and the logits of every step stay within the end-to-end bar of the fused=False model's."""
    import copy

    from bench import MXINT_Q
    from lqer_amd import attention as A
    from lqer_amd.models import load_low_rank_dict, quantize_model

    qc = {"linear": MXINT_Q, "matmul": CFG}
    model = quantize_model(F._tiny_llama(2 if family == "llama-gqa" else 4), qc, {"linear": {"rank": 16}})
    load_low_rank_dict(model, F._ab_dict(model, 16))
    unfused = A.enable_quantized_attention(copy.deepcopy(model), qc).to(DEV)
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV)
    real, seen = A.attention_flexible, []

    def recording(q, k, v, cfg0, cfg1, scaling, attention_mask=None, causal=False, **kw):
        seen.append((q.shape[2], real.kernel(q, k, v, cfg0, cfg1, attention_mask, causal)))
        return real(q, k, v, cfg0, cfg1, scaling, attention_mask=attention_mask, causal=causal, **kw)

    monkeypatch.setattr(A, "attention_flexible", recording)
    ids = torch.randint(0, 200, (2, 16), generator=torch.Generator().manual_seed(11)).to(DEV)

    def generate_logits(m):
        steps, past = [], None
        with torch.no_grad():
            out = m(input_ids=ids[:, :12], use_cache=True)
            steps.append(out.logits.float().cpu())
            past = out.past_key_values
            for i in range(12, 16):
                out = m(input_ids=ids[:, i:i + 1], past_key_values=past, use_cache=True)
                steps.append(out.logits.float().cpu())
                past = out.past_key_values
        return steps

    got = generate_logits(model)
    calls = list(seen)
    want = generate_logits(unfused)
    layers = model.config.num_hidden_layers
    assert len(calls) == 5 * layers, calls  # (the fused=False model never calls attention_flexible)
    assert all(kern == "prefill" for s, kern in calls[:layers]) and all(s == 12 for s, _ in calls[:layers])
    assert all(s == 1 and kern == "decode" for s, kern in calls[layers:]), calls
    for i, (g, w) in enumerate(zip(got, want)):
        err = F._rel(g, w)
        print(f"end to end {family} step {i}: logits vs fused=False {err:.3e}")
        assert torch.isfinite(g).all() and err <= 1e-4

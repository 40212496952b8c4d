"""The prefill kernel over the packed KV cache on the GPU (lqer_attention_q_kv: csrc/kv_cache.hip's k_kv_kimage / k_kv_vimage write the
two bf16 images from the cache's codes, csrc/attn_q.hip's k_attn_q runs on them; lqer_amd.kvcache.attention_flexible_cached(kernel=
"prefill"), lqer_amd.attention.quantized_kv_cache(chunked_prefill=True)).

The images hold what the raw image kernels write from the K and V that were appended, and the attention kernel is the same, so every
check here is an equality of bits against attention_flexible(..., kernel="prefill") on the raw tensors, whose own agreement with the
comparator tests/test_gpu_attention_fused.py establishes.  There is no tolerance in this file.

Shapes are the smallest that reach every edge: an open block of keys, one and several blocks of 16 d, a head dim that is no multiple of
32, more keys than one 64-key tile of either image kernel, two query tiles, grouped-query heads, exactly one closed block, one query
row, more query rows than keys - each over a cache with room to spare and over one with no row beyond the image's own padding."""
import ctypes as C

import pytest
import torch

import test_gpu_attention_decode as Dm
import test_gpu_attention_fused as F
import test_gpu_kv_cache as K

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES, DT_IDS = F.CFG, F.DEV, F.DTYPES, K.DT_IDS
_ids = lambda c: "x".join(map(str, c))
_bits = lambda x: x.contiguous().view(torch.uint8)


def _raw(q, k, v, scaling, **kw):
    from lqer_amd import attention_flexible

    return attention_flexible(q, k, v, CFG, CFG, scaling, kernel="prefill", **kw)


def _packed(q, cache, scaling, **kw):
    from lqer_amd import attention_flexible_cached

    return attention_flexible_cached(q, cache, scaling, kernel="prefill", **kw)


# ---- 1. the same bits as the prefill kernel on the raw tensors -------------------------------------------------------------------
SHAPES = [(1, 2, 1, 9, 25, 16), (2, 4, 2, 40, 77, 80), (1, 4, 4, 130, 200, 128), (1, 8, 2, 33, 300, 64), (2, 2, 2, 16, 16, 48),
          (1, 2, 1, 1, 37, 32), (1, 2, 2, 50, 20, 64)]
CASES = [(shape, mode) for shape in SHAPES for mode in ("none", "mask", "causal") if not (mode == "causal" and shape[3] > shape[4])]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape, mode", CASES, ids=[_ids(s) + "-" + m for s, m in CASES])
def test_same_bits_as_the_raw_prefill_kernel(dtype, shape, mode):
    b, h, hk, s, t, d = shape
    q, k, v = (x.to(DEV) for x in (F._randn((b, h, s, d), dtype, 10, 3.0), F._randn((b, hk, t, d), dtype, 11, 3.0), F._randn((b, hk, t, d), dtype, 12)))
    mask = Dm._mask(mode, b, s, t, dtype)
    mask = None if mask is None or mode == "causal" else mask.to(DEV)
    scaling, causal = d ** -0.5, mode == "causal"
    want = {layout: _raw(q, k, v, scaling, attention_mask=mask, causal=causal, out_layout=layout, return_stats=True) for layout in ("bhsd", "bshd")}
    pattern = [t - s, s] if t > s else None  # a prefill, then the chunk's append
    for capacity in (256, (t + 15) // 16 * 16):  # ... and no row of the cache behind the last block of keys
        cache = K._cache(k, v, pattern, capacity)
        assert cache.capacity >= t and (capacity == 256 or cache.capacity == capacity)
        snap = cache.buf.clone()
        for layout in ("bhsd", "bshd"):
            out, st = _packed(q, cache, scaling, attention_mask=mask, causal=causal, out_layout=layout, return_stats=True)
            ref, ref_st = want[layout]
            assert out.shape == ref.shape and out.dtype == dtype
            assert torch.equal(_bits(out), _bits(ref)), f"capacity {capacity} {layout}: {(out != ref).sum().item()} of {out.numel()} outputs differ"
            assert torch.equal(_bits(st), _bits(ref_st)), f"capacity {capacity} {layout}: row_stats differ"
        assert torch.equal(cache.buf, snap)
    assert torch.isfinite(out).all()


# ---- 2. a wide range of block exponents ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "causal"])
def test_wide_exponent_range_fp32(mode):
    """Blocks of K and V scaled by 2^40 and by 2^-40 (the latter all |x| <= 1e-8: flushed to zero at the append and by the raw image
    kernels alike), one tiny and one huge value inside ordinary blocks, an all-zero block and scattered zeros."""
    b, h, hk, s, t, d = 1, 2, 1, 20, 53, 48
    k, v = K._kv((b, hk, t, d), torch.float32, 300)
    k[:, :, :16, :8] *= 2.0 ** 40
    k[:, :, 16:32, 8:16] *= 2.0 ** -40
    k[:, :, 5, 20] *= 2.0 ** -40
    k[:, :, 32:, 24:32] *= 2.0 ** 40
    v[:, :, 3, :16] *= 2.0 ** 40
    v[:, :, 4, 16:32] *= 2.0 ** -40
    v[:, :, 6, 33] *= 2.0 ** -40
    v[:, :, 7, 40] *= 2.0 ** 40
    assert int(((k != 0) & (k.abs() <= 1e-8)).sum()) > 100 and float(k.abs().max()) > 2.0 ** 39
    q, k, v = F._randn((b, h, s, d), torch.float32, 301).to(DEV), k.to(DEV), v.to(DEV)
    want, want_st = _raw(q, k, v, d ** -0.5, causal=mode == "causal", return_stats=True)
    got, got_st = _packed(q, K._cache(k, v, [t - s, s]), d ** -0.5, causal=mode == "causal", return_stats=True)
    bad = (_bits(got).view(-1, 4) != _bits(want).view(-1, 4)).any(1).nonzero().flatten()
    first = int(bad[0]) if bad.numel() else 0
    assert bad.numel() == 0, (f"{bad.numel()} of {got.numel()} outputs differ; first at flat index {first}: packed {got.flatten()[first].item()!r}, "
                              f"raw {want.flatten()[first].item()!r}")
    assert torch.equal(_bits(got_st), _bits(want_st))
    assert torch.isfinite(want).all() and torch.isfinite(want_st).all()


# ---- 3. a prompt in chunks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_chunked_equals_one_shot(dtype):
    """192 tokens fed as chunks that are multiples of 16 (no block of keys is ever open when it is read: every block is quantized from
    the same 16 keys as in one shot, and the kernel treats query rows independently): the chunks' outputs are the one-shot output.
    Chunks of 40 leave an open block, quantized zero-padded: each chunk equals the raw kernel on the keys so far."""
    from lqer_amd import QuantizedKVCache

    b, h, hk, d, T = 1, 4, 2, 64, 192
    q, k, v = (x.to(DEV) for x in (F._randn((b, h, T, d), dtype, 20, 2.0), F._randn((b, hk, T, d), dtype, 21, 2.0), F._randn((b, hk, T, d), dtype, 22)))
    one_shot = _raw(q, k, v, 0.125, causal=True)
    for n in (64, 48, 40):
        cache, outs = QuantizedKVCache(b, hk, d, CFG, CFG, dtype, DEV), []
        for at in range(0, T, n):
            end = min(at + n, T)
            cache.append(k[:, :, at:end], v[:, :, at:end])
            outs.append(_packed(q[:, :, at:end], cache, 0.125, causal=True))
            if n % 16:
                want = _raw(q[:, :, at:end], k[:, :, :end], v[:, :, :end], 0.125, causal=True)
                assert torch.equal(_bits(outs[-1]), _bits(want)), f"chunks of {n}: the chunk ending at {end} differs from the raw kernel"
        assert cache.length == T
        if n % 16 == 0:
            got = torch.cat(outs, 2)
            assert torch.equal(_bits(got), _bits(one_shot)), f"chunks of {n}: {(got != one_shot).sum().item()} of {got.numel()} outputs differ"


# ---- 4. guard zones -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["mask", "causal"])
def test_guard_zones(dtype, mode):
    """q, the cache (exactly lqer_kv_cache_bytes, capacity 48: three blocks of keys, the last one open at T = 37), mask, out (rows padded:
    stride d + 8), row_stats and the workspace (exactly the reported size) between guards, over a pseudo-random fill and over 0xFF - NaN
    in every float type, 255 in every code and exponent, so whatever the call reads of the workspace or of the cache beyond what the
    appends wrote shows in the output - and once with q one element off a 16-byte boundary."""
    from _guard import guarded, rows_bytes

    from lqer_amd import _lib, ops

    b, h, hk, s, t, d = 2, 4, 2, 19, 37, 48
    capacity, steps = 48, [18, 19]
    esz = torch.empty(0, dtype=dtype).element_size()
    ld = d + 8
    q, k, v = F._randn((b, h, s, d), dtype, 60), F._randn((b, hk, t, d), dtype, 61), F._randn((b, hk, t, d), dtype, 62)
    mask = F._causal_mask(s, t, dtype, pad=Dm._pad(s, t), batch=b)
    L = _lib.lib()
    fmt = ops.make_qfmt(CFG["x_quantizer"], "x")
    tri = lambda *xs: (C.c_int64 * 3)(*xs)
    stream = torch.cuda.current_stream().cuda_stream
    ncache = L.lqer_kv_cache_bytes(ops.dtype_code(q), b, hk, capacity, d)
    nws = L.lqer_attention_q_kv_workspace_bytes(b, h, hk, s, t, d)
    assert ncache > 0 and nws == L.lqer_attention_q_workspace_bytes(b, h, hk, s, t, d) > 0
    results = []
    for fill, unaligned in ((0, False), (0xFF, False), (0xFF, True)):
        gc = guarded(ncache, fill=fill, name="cache")
        at = 0
        for n in steps:
            kn, vn = k[:, :, at:at + n].contiguous().to(DEV), v[:, :, at:at + n].contiguous().to(DEV)
            st3 = tri(hk * n * d, n * d, d)
            _lib.check(L.lqer_kv_cache_append(gc.ptr, ncache, kn.data_ptr(), vn.data_ptr(), st3, st3, ops.dtype_code(q), b, hk, capacity, d, at, n,
                                              C.byref(fmt), C.byref(fmt), stream), "lqer_kv_cache_append")
            at += n
        torch.cuda.synchronize()
        gc.check()
        gc.snapshot = gc.arena.clone()  # from here on the cache is an input
        qd = q.to(DEV)
        if unaligned:
            qv, qflat = K._shifted(qd)
            qsnap, qp = qflat.clone(), qv.data_ptr()
        else:
            gq = guarded(q.numel() * esz, fill=fill, name="q").load(qd)
            qp = gq.ptr
        gm = guarded(mask.numel() * esz, fill=fill, name="mask").load(mask.to(DEV))
        go = guarded(rows_bytes(b * h * s, d, ld, esz), row_pitch_bytes=ld * esz, fill=fill, name="out")
        gs = guarded(b * h * s * 2 * 4, fill=fill, name="row_stats")
        gw = guarded(nws, fill=fill, name="workspace")
        rc = L.lqer_attention_q_kv(qp, gc.ptr, ncache, capacity, gm.ptr if mode == "mask" else None, go.ptr, gs.ptr, ops.dtype_code(q), b, h, hk, s, t, d,
                                   tri(h * s * d, s * d, d), tri(s * t, 0, t) if mode == "mask" else None, tri(h * s * ld, s * ld, ld), 0.2,
                                   int(mode == "causal"), C.byref(fmt), C.byref(fmt), C.byref(fmt), C.byref(fmt), gw.ptr, nws, stream)
        _lib.check(rc, "lqer_attention_q_kv")
        torch.cuda.synchronize()
        gc.unchanged()  # the attention call does not write the cache
        gm.unchanged()
        if unaligned:
            assert torch.equal(qflat, qsnap)
        else:
            gq.unchanged()
        for gbuf in (go, gs, gw):
            gbuf.check()
        go.gaps_unchanged(b * h * s, d, ld, dtype)
        results.append((go.rows_view(b * h * s, d, ld, dtype).contiguous().clone(), gs.view(torch.float32).reshape(b, h, s, 2).clone()))
    for out, st in results[1:]:
        assert torch.equal(_bits(out), _bits(results[0][0])) and torch.equal(_bits(st), _bits(results[0][1]))
    # ... and those are the module's bits, which are the raw prefill kernel's
    dk, dv, dm = k.to(DEV), v.to(DEV), mask.to(DEV) if mode == "mask" else None
    mod, mod_st = _packed(q.to(DEV), K._cache(dk, dv, steps, capacity), 0.2, attention_mask=dm, causal=mode == "causal", return_stats=True)
    raw, raw_st = _raw(q.to(DEV), dk, dv, 0.2, attention_mask=dm, causal=mode == "causal", return_stats=True)
    got, got_st = results[0][0].reshape(b, h, s, d), results[0][1]
    assert torch.equal(_bits(got), _bits(mod)) and torch.equal(_bits(got_st), _bits(mod_st))
    assert torch.equal(_bits(got), _bits(raw)) and torch.equal(_bits(got_st), _bits(raw_st))


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay():
    from lqer_amd.graph import GraphedCallable

    dtype, (b, h, hk, s, t, d) = torch.float16, (1, 4, 2, 12, 44, 64)
    k, v = F._randn((b, hk, t, d), dtype, 71).to(DEV), F._randn((b, hk, t, d), dtype, 72).to(DEV)
    cache = K._cache(k, v, [t - s, s])
    fn = lambda q: _packed(q, cache, 0.125, causal=True, out_layout="bshd")
    mk = lambda seed: F._randn((b, h, s, d), dtype, seed).to(DEV)
    step = GraphedCallable(fn, mk(70).clone(), warmup=2)  # (captures under torch.cuda.graph)
    outs = []
    for seed in (80, 90):
        q = mk(seed)
        want = fn(q)
        got = step(q).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        outs.append(got)
    assert not torch.equal(outs[0], outs[1])
    assert torch.equal(outs[1], _raw(mk(90), k, v, 0.125, causal=True, out_layout="bshd"))


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["llama", "llama-gqa", "opt"])
def test_end_to_end_second_turn(family, monkeypatch):
    """Batch 2: a 20-token prompt, a 12-token second turn on the non-empty cache, 5 greedy steps of one token.  With
    quantized_kv_cache(model, chunked_prefill=True) the logits of every forward equal those of a DynamicCache run of the same calls (whose
    second turn takes the prefill kernel on the raw K and V, whose steps take the decode kernel); the default cache still refuses."""
    from transformers import DynamicCache

    model, qc, A = K._model(family)
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV)
    real, real_cached, seen = A.attention_flexible, A.attention_flexible_cached, []

    def rec_raw(q, k, v, cfg0, cfg1, scaling, attention_mask=None, causal=False, **kw):
        seen.append(("raw", q.shape[2], real.kernel(q, k, v, cfg0, cfg1, attention_mask, causal)))
        return real(q, k, v, cfg0, cfg1, scaling, attention_mask=attention_mask, causal=causal, **kw)

    def rec_cached(q, cache, scaling, **kw):
        seen.append(("packed", q.shape[2], cache.length, kw.get("kernel")))
        return real_cached(q, cache, scaling, **kw)

    monkeypatch.setattr(A, "attention_flexible", rec_raw)
    monkeypatch.setattr(A, "attention_flexible_cached", rec_cached)
    ids = torch.randint(0, 200, (2, 32), generator=torch.Generator().manual_seed(11)).to(DEV)

    def run(past):
        logits = []
        with torch.no_grad():
            for tok in (ids[:, :20], ids[:, 20:]):
                logits.append(model(input_ids=tok, past_key_values=past, use_cache=True).logits)
            for _ in range(5):
                tok = logits[-1][:, -1:].argmax(-1)
                logits.append(model(input_ids=tok, past_key_values=past, use_cache=True).logits)
        return logits

    packed = A.quantized_kv_cache(model, chunked_prefill=True)
    got = run(packed)
    calls, layers = list(seen), model.config.num_hidden_layers
    del seen[:]
    dyn = DynamicCache()
    want = run(dyn)
    assert [c[:2] for c in calls[:layers]] == [("raw", 20)] * layers  # the first prompt attends over its own raw K and V
    assert calls[layers:2 * layers] == [("packed", 12, 32, "prefill")] * layers
    assert calls[2 * layers:] == [("packed", 1, 33 + i, None) for i in range(5) for _ in range(layers)]
    assert seen[layers:2 * layers] == [("raw", 12, "prefill")] * layers and all(c == ("raw", 1, "decode") for c in seen[2 * layers:])
    assert len(seen) == 7 * layers
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), f"forward {i}: {(g != w).sum().item()} of {g.numel()} logits differ"
    assert packed.get_seq_length() == dyn.get_seq_length() == 37
    # the default is unchanged
    past = A.quantized_kv_cache(model)
    with torch.no_grad():
        model(input_ids=ids[:, :20], past_key_values=past, use_cache=True)
        with pytest.raises(NotImplementedError, match="new tokens"):
            model(input_ids=ids[:, 20:], past_key_values=past, use_cache=True)

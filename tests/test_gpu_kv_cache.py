"""The packed KV cache on the GPU (lqer_kv_cache_append / lqer_attention_q_decode_kv / lqer_kv_cache_unpack; csrc/kv_cache.hip,
csrc/attn_decode.hip with the packed operand source; lqer_amd.kvcache, lqer_amd.attention.quantized_kv_cache).

What the cache stores is the output of the two quantizers the decode kernel applies to K and V, so every check here is an equality
of bits: the stored values against the oracle's block quantizer, every way of building a cache against every other, and the
attention over the cache against the decode kernel on the raw tensors (lqer_attention_q_decode), whose own agreement with the
comparator tests/test_gpu_attention_decode.py establishes.  The one tolerance is that file's bar, for one case per dtype.

Shapes are the smallest that reach every edge: T = 1, below / at / above one block of 16 keys, a ragged last block, several chunks,
one key past a power of two, and lengths at which the open block is exactly full (16, 32, 2048)."""
import ctypes as C

import pytest
import torch

import test_gpu_attention_decode as Dm
import test_gpu_attention_fused as F

pytestmark = pytest.mark.gpu

CFG, DEV, BAR, DTYPES = F.CFG, F.DEV, F.BAR, F.DTYPES
DT_IDS = ["f16", "bf16", "f32"]
_ids = lambda c: "x".join(map(str, c))


def _cache(k, v, pattern=None, capacity=256):
    """A QuantizedKVCache holding k / v [b, hk, T, d] (device tensors), appended in pieces of the given sizes (default: one call)."""
    from lqer_amd import QuantizedKVCache

    b, hk, t, d = k.shape
    cache = QuantizedKVCache(b, hk, d, CFG, CFG, k.dtype, k.device, capacity=capacity)
    at = 0
    for n in (pattern or [t]):
        cache.append(k[:, :, at:at + n], v[:, :, at:at + n])
        at += n
    assert at == t == cache.length
    return cache


def _oracle(k, v):
    """Q_w0 on K^T [b hk, d, T] (blocks of 16 along t) and Q_w1 on V [b hk, T, d] (along d), fp32, as [b, hk, T, d]."""
    from oracle import lqer_oracle as O

    b, hk, t, d = k.shape
    kq = O.mxint_quantize(k.float().reshape(b * hk, t, d).transpose(1, 2).contiguous(), width=8, block_size=[1, 16])
    vq = O.mxint_quantize(v.float().reshape(b * hk, t, d), width=8, block_size=[1, 16])
    return kq.transpose(1, 2).reshape(b, hk, t, d), vq.reshape(b, hk, t, d)


def _kv(shape, dtype, seed, sc=1.0):
    """randn x sc with one all-zero block of keys (16 keys at one d), one all-zero block of a V row, and scattered exact zeros."""
    b, hk, t, d = shape
    k, v = F._randn(shape, dtype, seed, sc), F._randn(shape, dtype, seed + 1, sc)
    k[:, :, (16 if t >= 32 else 0):(32 if t >= 32 else 16), 3] = 0
    v[:, :, t // 2, 16 * ((d // 16) - 1):] = 0
    g = torch.Generator().manual_seed(seed + 2)
    k[torch.rand(shape, generator=g) < 0.02] = 0
    v[torch.rand(shape, generator=g) < 0.02] = 0
    return k, v


# ---- 1. the stored values against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sc", [1.0, 3.0])
@pytest.mark.parametrize("t", [1, 15, 16, 17, 37, 300])
def test_stored_values_equal_the_oracle(dtype, sc, t):
    shape = (2, 2, t, 128 if t == 300 else 48)
    k, v = _kv(shape, dtype, 200 + t, sc)
    want_k, want_v = _oracle(k, v)
    cache = _cache(k.to(DEV), v.to(DEV), [min(t, 5)] + ([t - 5] if t > 5 else []))
    got_k, got_v = (x.cpu() for x in cache.dequantized())
    assert got_k.dtype == torch.float32 and got_k.shape == shape
    assert torch.equal(got_k, want_k), f"K: {(got_k != want_k).sum().item()} of {want_k.numel()} differ"
    assert torch.equal(got_v, want_v), f"V: {(got_v != want_v).sum().item()} of {want_v.numel()} differ"


def test_stored_values_far_magnitudes_fp32():
    """Blocks near 2^100 and near 2^-100 (and both in one block).  Every magnitude near 2^-100 is a non-zero |x| <= 1e-8, which the
    reference passes through untouched and the HIP path flushes to zero (the declared difference, csrc/qmm_image.h): the expected
    values are the oracle's for the input with exactly those elements set to zero - everything else bit for bit."""
    shape = (1, 2, 37, 48)
    k, v = _kv(shape, torch.float32, 300)
    k[:, :, :16, :8] *= 2.0 ** 100
    k[:, :, 16:32, 8:16] *= 2.0 ** -100
    k[:, :, 5, 20] *= 2.0 ** -100   # one tiny value inside an ordinary block
    k[:, :, 32:, 24:32] *= 2.0 ** 100
    v[:, :, 3, :16] *= 2.0 ** 100
    v[:, :, 4, 16:32] *= 2.0 ** -100
    v[:, :, 6, 33] *= 2.0 ** -100
    v[:, :, 7, 40] *= 2.0 ** 100    # one huge value inside an ordinary block
    flush = lambda x: torch.where(x.abs() <= 1e-8, torch.zeros_like(x), x)
    assert int(((k != 0) & (k.abs() <= 1e-8)).sum()) > 200 and float(k.abs().max()) > 2.0 ** 99
    want_k, want_v = _oracle(flush(k), flush(v))
    got_k, got_v = (x.cpu() for x in _cache(k.to(DEV), v.to(DEV), [17, 20]).dequantized())
    assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v)


# ---- 2. append patterns give one cache ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("t", [37, 300])
def test_append_patterns_and_capacities_give_one_cache(dtype, t):
    from lqer_amd import attention_flexible_cached

    b, h, hk, s, d = 2, 4, 2, 2, 64
    k, v = (x.to(DEV) for x in _kv((b, hk, t, d), dtype, 400 + t, 2.0))
    q = F._randn((b, h, s, d), dtype, 402).to(DEV)
    builds = {"one call": ([t], 256), "singles": ([1] * t, 256), "16 then singles": ([16] + [1] * (t - 16), 256),
              "5, 27, singles": ([5, 27] + [1] * (t - 32), 256), "capacity 48": ([t], 48), "capacity 64": ([5, t - 5], 64),
              "capacity 4096": ([t], 4096), "grown from 16": ([7] + [1] * 12 + [t - 19], 16)}
    ref = None
    for name, (pattern, capacity) in builds.items():
        cache = _cache(k, v, pattern, capacity)
        assert cache.capacity >= t and cache.capacity % 16 == 0
        if name == "grown from 16":
            assert cache.capacity == 16 * 2 ** ((t - 1) // 16).bit_length()
        kq, vq = cache.dequantized()
        out, st = attention_flexible_cached(q, cache, d ** -0.5, causal=True, return_stats=True)
        if ref is None:
            ref = (kq, vq, out, st)
            continue
        for what, a, r in zip(("K", "V", "attention", "row_stats"), (kq, vq, out, st), ref):
            assert torch.equal(a.view(torch.uint8), r.view(torch.uint8)), f"{name}: {what} differs from the one-call cache"
    cache.reset()
    assert cache.length == 0
    cache.append(k[:, :, :9], v[:, :, :9])
    assert torch.equal(cache.dequantized()[0], _cache(k[:, :, :9], v[:, :, :9]).dequantized()[0])  # (a reset cache starts over)


# ---- 2b. the bytes an append leaves behind ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_append_steps_leave_the_bytes_of_one_append(dtype):
    """One cache of capacity 80 through appends of 5, 11, 1, 40, 7 and 3 keys - inside the open block, up to its end, from a boundary,
    across three further blocks from a non-empty open block, across one, from a boundary again.  After every step (a) the bytes of every
    section's blocks below ceil(length / 16) are those of a cache that got the same keys in ONE append (both buffers start from the same
    bytes, so what neither writes - V rows at and beyond the length - compares too), and (b) staging row t % 16 holds the raw bits of K
    row t for every t of the open block.  The buffers lie between guard zones."""
    from _guard import guarded

    from lqer_amd import QuantizedKVCache, kvcache

    b, hk, d, capacity = 2, 2, 48, 80
    z, bits = b * hk, torch.int16 if dtype == torch.float16 else torch.int32
    k, v = (x.to(DEV) for x in _kv((b, hk, 67, d), dtype, 500))
    sections, total = kvcache._sections(dtype, b, hk, capacity, d)

    def cache_on_guard():
        g = guarded(total, name="cache")
        c = QuantizedKVCache(b, hk, d, CFG, CFG, dtype, DEV, capacity=capacity)
        assert c.capacity == capacity and c.buf.numel() == total
        c.buf = g.payload
        return c, g

    cache, guard = cache_on_guard()
    for before, n in ((0, 5), (5, 11), (16, 1), (17, 40), (57, 7), (64, 3)):
        assert cache.length == before
        cache.append(k[:, :, before:before + n], v[:, :, before:before + n])
        length = before + n
        fresh, fresh_guard = cache_on_guard()
        fresh.append(k[:, :, :length], v[:, :, :length])
        torch.cuda.synchronize()
        for gz in (guard, fresh_guard):
            gz.check()
        assert cache.buf.data_ptr() == guard.ptr
        blocks = (length + 15) // 16
        for name, at, per_block in sections[:4]:
            row = (capacity // 16) * per_block
            got, want = (c.buf[at:at + z * row].view(z, row)[:, :blocks * per_block] for c in (cache, fresh))
            assert torch.equal(got, want), f"{before} + {n}: {name}: {(got != want).sum().item()} bytes differ from the one-append cache"
        name, at, _ = sections[4]
        assert name == "k_stage"
        stage = cache.buf[at:at + z * 16 * d * k.element_size()].view(bits).view(z, 16, d)
        for t in range(length // 16 * 16, length):
            assert torch.equal(stage[:, t % 16], k[:, :, t].reshape(z, d).view(bits)), f"{before} + {n}: staging row {t % 16} is not K row {t}"


# ---- 3. the same bits as the decode kernel on the raw tensors ------------------------------------------------------------------
SHAPES = Dm.PARITY + [(2, 4, 2, 1, 16, 48), (2, 8, 2, 3, 32, 64), (1, 4, 2, 1, 2048, 128)]


def _both(q, k, v, cache, scaling, mask, causal, layout):
    from lqer_amd import attention_flexible, attention_flexible_cached

    got = attention_flexible_cached(q, cache, scaling, attention_mask=mask, causal=causal, out_layout=layout, return_stats=True)
    want = attention_flexible(q, k, v, CFG, CFG, scaling, attention_mask=mask, causal=causal, out_layout=layout, return_stats=True, kernel="decode")
    return got, want


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["none", "mask", "causal"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_same_bits_as_the_raw_decode_kernel(dtype, mode, shape):
    b, h, hk, s, t, d = shape
    q, k, v = (x.to(DEV) for x in (F._randn((b, h, s, d), dtype, 10, 3.0), F._randn((b, hk, t, d), dtype, 11, 3.0), F._randn((b, hk, t, d), dtype, 12)))
    mask = Dm._mask(mode, b, s, t, dtype)
    mask = None if mask is None or mode == "causal" else mask.to(DEV)
    cache = _cache(k, v, [t - 1, 1] if t > 1 else None)  # a prefill, then one step's append
    snap = cache.buf.clone()
    for layout in ("bhsd", "bshd"):
        (out, st), (want, want_st) = _both(q, k, v, cache, d ** -0.5, mask, mode == "causal", layout)
        assert out.shape == want.shape and out.dtype == dtype
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), f"{layout}: {(out != want).sum().item()} of {out.numel()} outputs differ"
        assert torch.equal(st.view(torch.uint8), want_st.view(torch.uint8)), f"{layout}: row_stats differ"
    assert torch.isfinite(out).all() and torch.equal(cache.buf, snap)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_parity_vs_comparator(dtype):
    """One representative case per dtype against the comparator at the decode kernel's bar (tests/test_gpu_attention_decode.py)."""
    from lqer_amd import attention_flexible_cached

    b, h, hk, s, t, d = 2, 4, 2, 5, 37, 80
    q, k, v = F._randn((b, h, s, d), dtype, 10, 3.0), F._randn((b, hk, t, d), dtype, 11, 3.0), F._randn((b, hk, t, d), dtype, 12)
    mask = Dm._mask("mask", b, s, t, dtype)
    ref, _, _ = F.comparator(q, k, v, d ** -0.5, mask)
    got = attention_flexible_cached(q.to(DEV), _cache(k.to(DEV), v.to(DEV), [30, 7]), d ** -0.5, attention_mask=mask.to(DEV))
    err = F._rel(got.cpu(), ref)
    print(f"packed cache vs comparator {dtype}: O rel-L2 {err:.3e}")
    assert torch.isfinite(got).all() and err <= BAR


def test_python_refusals():
    from lqer_amd import attention_flexible_cached

    dtype, (b, h, hk, t, d) = torch.float16, (1, 4, 2, 40, 64)
    k, v = F._randn((b, hk, t, d), dtype, 1).to(DEV), F._randn((b, hk, t, d), dtype, 2).to(DEV)
    cache = _cache(k, v)
    with pytest.raises(ValueError, match="query rows"):
        attention_flexible_cached(F._randn((b, h, 9, d), dtype, 3).to(DEV), cache, 0.125)
    with pytest.raises(ValueError):
        attention_flexible_cached(F._randn((b, h, 1, d), torch.bfloat16, 3).to(DEV), cache, 0.125)  # another dtype than the cache's
    with pytest.raises(ValueError):
        attention_flexible_cached(F._randn((b, 3, 1, d), dtype, 3).to(DEV), cache, 0.125)  # heads no multiple of the kv heads
    with pytest.raises(ValueError):
        cache.append(k[:, :1], v[:, :1])  # another number of kv heads
    assert cache.length == t


# ---- 4. guard zones -----------------------------------------------------------------------------------------------------------
def _shifted(x):
    """x's values in a view one element off a 16-byte boundary (rows that take the element-load path), and its storage."""
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device=x.device)
    flat[1:] = x.reshape(-1)
    y = flat[1:].view(x.shape)
    assert y.data_ptr() % 16 != 0
    return y, flat


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["mask", "causal"])
def test_guard_zones(dtype, mode):
    """The cache (exactly lqer_kv_cache_bytes), out (rows padded: stride d + 8), row_stats and the workspace between guards, over a
    pseudo-random fill and over 0xFF (NaN in every float type, 255 in every code: nothing may read rows beyond the length).  Appends
    of 21, 1, 1, 5 and 7 keys - inside the open block, up to its end, and across it from a non-empty open block (the append reads and rewrites staging rows in one launch)."""
    from _guard import guarded, rows_bytes

    from lqer_amd import _lib, ops

    b, h, hk, s, t, d = 2, 4, 2, 3, 35, 48
    capacity, steps = 40, [21, 1, 1, 5, 7]
    esz = torch.empty(0, dtype=dtype).element_size()
    ld = d + 8
    q, k, v = F._randn((b, h, s, d), dtype, 60), F._randn((b, hk, t, d), dtype, 61), F._randn((b, hk, t, d), dtype, 62)
    mask = F._causal_mask(s, t, dtype, pad=Dm._pad(s, t), batch=b)
    L = _lib.lib()
    fmt = ops.make_qfmt(CFG["x_quantizer"], "x")
    tri = lambda *xs: (C.c_int64 * 3)(*xs)
    stream = torch.cuda.current_stream().cuda_stream
    ncache = L.lqer_kv_cache_bytes(ops.dtype_code(q), b, hk, capacity, d)
    nws = L.lqer_attention_q_decode_kv_workspace_bytes(b, h, hk, s, t, d)
    assert ncache > 0 and nws > 0
    results = []
    for fill, unaligned in ((0, False), (0xFF, False), (0xFF, True)):
        gc = guarded(ncache, fill=fill, name="cache")
        at = 0
        for n in steps:
            kn, vn = k[:, :, at:at + n].contiguous().to(DEV), v[:, :, at:at + n].contiguous().to(DEV)
            if unaligned:
                (kn, kflat), (vn, vflat) = _shifted(kn), _shifted(vn)
                snaps = (kflat.clone(), vflat.clone())
                kp, vp = kn.data_ptr(), vn.data_ptr()
            else:
                gk = guarded(kn.numel() * esz, fill=fill, name="k_new").load(kn)
                gv = guarded(vn.numel() * esz, fill=fill, name="v_new").load(vn)
                kp, vp = gk.ptr, gv.ptr
            st3 = tri(hk * n * d, n * d, d)
            _lib.check(L.lqer_kv_cache_append(gc.ptr, ncache, kp, vp, st3, st3, ops.dtype_code(q), b, hk, capacity, d, at, n, C.byref(fmt), C.byref(fmt),
                                              stream), "lqer_kv_cache_append")
            torch.cuda.synchronize()
            gc.check()
            if unaligned:
                assert torch.equal(kflat, snaps[0]) and torch.equal(vflat, snaps[1])
            else:
                gk.unchanged()
                gv.unchanged()
            at += n
        assert at == t
        gc.snapshot = gc.arena.clone()  # from here on the cache is an input
        qd = q.to(DEV)
        if unaligned:
            qv, qflat = _shifted(qd)
            qsnap, qp = qflat.clone(), qv.data_ptr()
        else:
            gq = guarded(q.numel() * esz, fill=fill, name="q").load(qd)
            qp = gq.ptr
        gm = guarded(mask.numel() * esz, fill=fill, name="mask").load(mask.to(DEV))
        go = guarded(rows_bytes(b * h * s, d, ld, esz), row_pitch_bytes=ld * esz, fill=fill, name="out")
        gs = guarded(b * h * s * 2 * 4, fill=fill, name="row_stats")
        gw = guarded(nws, fill=fill, name="workspace")
        rc = L.lqer_attention_q_decode_kv(qp, gc.ptr, ncache, capacity, gm.ptr if mode == "mask" else None, go.ptr, gs.ptr, ops.dtype_code(q), b, h, hk,
                                          s, t, d, tri(h * s * d, s * d, d), tri(s * t, 0, t) if mode == "mask" else None, tri(h * s * ld, s * ld, ld), 0.2,
                                          int(mode == "causal"), C.byref(fmt), C.byref(fmt), C.byref(fmt), C.byref(fmt), gw.ptr, nws, stream)
        _lib.check(rc, "lqer_attention_q_decode_kv")
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
        assert torch.equal(out.view(torch.uint8), results[0][0].view(torch.uint8)) and torch.equal(st, results[0][1])
    # ... and those are the bits of the decode kernel on the raw tensors
    from lqer_amd import attention_flexible

    want, want_st = attention_flexible(q.to(DEV), k.to(DEV), v.to(DEV), CFG, CFG, 0.2, attention_mask=mask.to(DEV) if mode == "mask" else None,
                                       causal=mode == "causal", return_stats=True, kernel="decode")
    assert torch.equal(results[0][0].reshape(b, h, s, d), want) and torch.equal(results[0][1], want_st)


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("len0, n", [(27, 1), (32, 3), (30, 3)], ids=["inside the open block", "from a block boundary", "across a block boundary"])
def test_graph_capture_and_replay(len0, n):
    """Appends at fixed lengths plus the attention call, captured and replayed on new q / k_new / v_new, against the eager calls on a
    second cache.  The captured step starts from length 0 - the len0 past keys, then the n new ones - because an append that leaves a
    non-empty open block overwrites the staging rows it read (30 + 3) and cannot be repeated at the same length."""
    from lqer_amd import attention_flexible_cached
    from lqer_amd.graph import GraphedCallable

    dtype, (b, h, hk, d) = torch.float16, (1, 4, 2, 64)
    k0, v0 = F._randn((b, hk, len0, d), dtype, 68).to(DEV), F._randn((b, hk, len0, d), dtype, 69).to(DEV)
    mk = lambda seed: [x.to(DEV) for x in (F._randn((b, h, n, d), dtype, seed), F._randn((b, hk, n, d), dtype, seed + 1), F._randn((b, hk, n, d), dtype, seed + 2))]

    def step_on(cache):
        def fn(q, kn, vn):
            cache.reset()
            cache.append(k0, v0)
            cache.append(kn, vn)
            return attention_flexible_cached(q, cache, 0.125, causal=True, out_layout="bshd")
        return fn

    graphed, eager = step_on(_cache(k0, v0)), step_on(_cache(k0, v0))
    static = [x.clone() for x in mk(70)]
    step = GraphedCallable(graphed, *static, warmup=2)
    outs = []
    for seed in (70, 80, 90):
        new = mk(seed)
        want = eager(*new)
        got = step(*new).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        outs.append(got)
    assert not torch.equal(outs[0], outs[1])
    from lqer_amd import attention_flexible

    q, kn, vn = mk(90)
    raw = attention_flexible(q, torch.cat([k0, kn], 2), torch.cat([v0, vn], 2), CFG, CFG, 0.125, causal=True, out_layout="bshd", kernel="decode")
    assert torch.equal(outs[2], raw)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------
def _model(family):
    from bench import MXINT_Q, OPT_Q
    from lqer_amd import attention as A
    from lqer_amd.models import load_low_rank_dict, quantize_model

    lin_q = OPT_Q if family == "opt" else MXINT_Q
    qc = {"linear": lin_q, ("bmm" if family == "opt" else "matmul"): CFG}
    base = F._tiny_opt() if family == "opt" else F._tiny_llama(2 if family == "llama-gqa" else 4)
    model = quantize_model(base, qc, {"linear": {"rank": 16}})
    load_low_rank_dict(model, F._ab_dict(model, 16))
    return model, qc, A


@pytest.mark.parametrize("family", ["llama", "llama-gqa", "opt"])
def test_end_to_end_generation(family, monkeypatch):
    """Batch 2, a 20-token prompt, 20 greedy steps of one token (across the block boundary at 32): with the packed cache the logits of
    every step equal those of a DynamicCache run, whose decode steps take the decode kernel on the raw K and V."""
    from transformers import DynamicCache

    model, qc, A = _model(family)
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV)
    real, real_cached, seen = A.attention_flexible, A.attention_flexible_cached, []

    def rec_raw(q, k, v, cfg0, cfg1, scaling, attention_mask=None, causal=False, **kw):
        seen.append(("raw", q.shape[2], real.kernel(q, k, v, cfg0, cfg1, attention_mask, causal)))
        return real(q, k, v, cfg0, cfg1, scaling, attention_mask=attention_mask, causal=causal, **kw)

    def rec_cached(q, cache, scaling, **kw):
        seen.append(("packed", q.shape[2], cache.length))
        return real_cached(q, cache, scaling, **kw)

    monkeypatch.setattr(A, "attention_flexible", rec_raw)
    monkeypatch.setattr(A, "attention_flexible_cached", rec_cached)
    ids = torch.randint(0, 200, (2, 20), generator=torch.Generator().manual_seed(11)).to(DEV)

    def run(past):
        logits, tok = [], ids
        with torch.no_grad():
            for _ in range(21):
                out = model(input_ids=tok, past_key_values=past, use_cache=True)
                logits.append(out.logits)
                tok = out.logits[:, -1:].argmax(-1)
        return logits

    packed = A.quantized_kv_cache(model)
    got = run(packed)
    calls, layers = list(seen), model.config.num_hidden_layers
    del seen[:]
    dyn = DynamicCache()
    want = run(dyn)
    assert [c[:2] for c in calls[:layers]] == [("raw", 20)] * layers  # the prefill attends over its own raw K and V
    assert calls[layers:] == [("packed", 1, 21 + i) for i in range(20) for _ in range(layers)]
    assert all(c == ("raw", 1, "decode") for c in seen[layers:]) and len(seen) == 21 * layers  # the reference run: the raw decode kernel
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"step {i}: {(g != w).sum().item()} of {g.numel()} logits differ"
    assert packed.get_seq_length() == dyn.get_seq_length() == 40
    capacity = packed.layers[0].cache.capacity
    dyn_bytes = sum(2 * l.keys[:, :, :1].numel() * capacity * l.keys.element_size() for l in dyn.layers)
    nbytes = sum(l.nbytes for l in packed.layers)
    print(f"end to end {family}: packed cache {nbytes} B against {dyn_bytes} B of K + V at capacity {capacity}")
    assert 0 < nbytes < dyn_bytes


def test_end_to_end_refusals():
    model, qc, A = _model("llama")
    eager = A.enable_quantized_attention(model, qc).to(DEV)
    with pytest.raises(ValueError, match="lqer_fused"):
        A.quantized_kv_cache(eager)
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV)
    past = A.quantized_kv_cache(model)
    ids = torch.randint(0, 200, (2, 29), generator=torch.Generator().manual_seed(12)).to(DEV)
    with torch.no_grad():
        model(input_ids=ids[:, :20], past_key_values=past, use_cache=True)
        with pytest.raises(NotImplementedError, match="new tokens"):
            model(input_ids=ids[:, 20:29], past_key_values=past, use_cache=True)  # a 9-token chunk on a non-empty cache
    # the attention function itself, handed tagged tensors by a caller that wants what only the unfused route has
    layer = past.layers[1]
    b, hk, d = layer.cache.batch, layer.cache.kv_heads, layer.cache.head_dim
    kn = torch.zeros(b, hk, 1, d, device=DEV)
    k1, v1 = layer.update(kn, kn.clone())
    q1 = torch.zeros(b, 4, 1, d, device=DEV)
    mod = model.model.layers[1].self_attn
    with pytest.raises(NotImplementedError):
        A.lqer_fused_attention_forward(mod, q1, k1, v1, None, 0.125, output_attentions=True)
    with pytest.raises(NotImplementedError):
        A.lqer_fused_attention_forward(mod, q1, k1, v1, torch.zeros(b, 1, 1, layer.cache.length, dtype=torch.float64, device=DEV), 0.125)

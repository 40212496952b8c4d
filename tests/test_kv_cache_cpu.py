"""The packed KV cache (csrc/kv_cache.hip, csrc/kv_pack.h, lqer_amd/kvcache.py), the part that needs no GPU: the five C-ABI exports are
declared, exported and bound, the byte count follows the header's layout, every refusal comes with its code and a message before
anything touches the device, and the Python side tells what the cache covers."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from lqer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
CFG = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
NEW = ("lqer_kv_cache_bytes", "lqer_kv_cache_append", "lqer_kv_cache_unpack", "lqer_attention_q_decode_kv_workspace_bytes",
       "lqer_attention_q_decode_kv")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    assert "#define LQER_ABI_VERSION 14" in hdr
    # lqer_attention_q_decode's argument list with (k, v) -> (cache, cache_bytes, capacity) and without their two stride arrays
    dec, kv = _lib.SIGNATURES["lqer_attention_q_decode"][1], _lib.SIGNATURES["lqer_attention_q_decode_kv"][1]
    assert kv == dec[:1] + [C.c_void_p, C.c_size_t, C.c_int64] + dec[3:14] + dec[16:]  # (dec[14], dec[15]: k_strides, v_strides)
    assert _lib.SIGNATURES["lqer_attention_q_decode_kv_workspace_bytes"] == _lib.SIGNATURES["lqer_attention_q_decode_workspace_bytes"]


def _layout_sum(esz, batch, kv, capacity, D):
    """include/lqer_hip.h: cap = capacity rounded up to 16; K codes [Z][cap][D], K exponents [Z][cap/16][D], V codes [Z][cap][D], V exponents
    [Z][cap/16][D/16][16] (one byte each), K staging [Z][16][D] of the dtype; each rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256
    cap, z = (capacity + 15) // 16 * 16, batch * kv
    return up(z * cap * D) + up(z * (cap // 16) * D) + up(z * cap * D) + up(z * (cap // 16) * (D // 16) * 16) + up(z * 16 * D * esz)


def test_cache_bytes():
    L = _lib.lib()
    for dt, esz in ((_lib.F16, 2), (_lib.BF16, 2), (_lib.F32, 4)):
        for batch, kv, capacity, D in [(1, 32, 2048, 128), (2, 3, 37, 48), (3, 1, 16, 16)]:  # (37: not a multiple of 16)
            assert L.lqer_kv_cache_bytes(dt, batch, kv, capacity, D) == _layout_sum(esz, batch, kv, capacity, D)
    assert L.lqer_kv_cache_bytes(_lib.F16, 1, 32, 33, 128) == L.lqer_kv_cache_bytes(_lib.F16, 1, 32, 48, 128)
    # the issue's arithmetic: 2 D (1 + 1/16) = 272 bytes per token and kv head at D = 128, plus the staging rows
    assert L.lqer_kv_cache_bytes(_lib.F16, 1, 32, 2048, 128) == 32 * 2048 * 272 + 32 * 16 * 128 * 2
    for bad in [(7, 1, 1, 16, 16), (_lib.F16, 0, 1, 16, 16), (_lib.F16, 1, 1, 0, 16), (_lib.F16, 1, 1, 16, 24), (_lib.F16, 1, 1, 16, 144)]:
        assert L.lqer_kv_cache_bytes(*bad) == 0


def _fmt(block=16, width=8, kind=_lib.Q_MXINT):
    return _lib.QFmt(kind, width, block, 8, 127)


MINIFLOAT = _lib.QFmt(_lib.Q_MINIFLOAT, 8, 16, 4, 7)
tri = lambda a, b, c: (C.c_int64 * 3)(a, b, c)


def _append(cache=0x100000, cache_bytes=None, k=0x20000, v=0x30000, ks=True, vs=True, dtype=_lib.F16, batch=1, kv=4, capacity=64, D=64, length=5, n=3,
            k_fmt=None, v_fmt=None):
    L = _lib.lib()
    k_fmt, v_fmt = k_fmt or _fmt(), v_fmt or _fmt()
    if cache_bytes is None:
        cache_bytes = 1 << 24
    st = tri(kv * n * D, n * D, D)
    rc = L.lqer_kv_cache_append(cache, cache_bytes, k, v, st if ks else None, st if vs else None, dtype, batch, kv, capacity, D, length, n,
                                C.byref(k_fmt) if k_fmt != "null" else None, C.byref(v_fmt) if v_fmt != "null" else None, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("len + n > capacity", dict(length=60, n=5), E_INVALID),
    ("n > capacity", dict(length=0, n=65), E_INVALID),
    ("n = 0", dict(n=0), E_INVALID),
    ("negative n", dict(n=-1), E_INVALID),
    ("negative len", dict(length=-1), E_INVALID),
    ("negative batch", dict(batch=-1), E_INVALID),
    ("kv_heads = 0", dict(kv=0), E_INVALID),
    ("capacity = 0", dict(capacity=0, length=0, n=1), E_INVALID),
    ("null cache", dict(cache=None), E_INVALID),
    ("cache not 16-byte aligned", dict(cache=0x100008), E_INVALID),
    ("short cache", dict(cache_bytes=_layout_sum(2, 1, 4, 64, 64) - 1), E_INVALID),
    ("null k_new", dict(k=None), E_INVALID),
    ("null v_new", dict(v=None), E_INVALID),
    ("null k strides", dict(ks=False), E_INVALID),
    ("null v strides", dict(vs=False), E_INVALID),
    ("null k format", dict(k_fmt="null"), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    ("block 32", dict(k_fmt=_fmt(32)), E_UNSUPPORTED),
    ("V block 32", dict(v_fmt=_fmt(32)), E_UNSUPPORTED),
    ("width 12", dict(v_fmt=_fmt(width=12)), E_UNSUPPORTED),
    ("minifloat", dict(k_fmt=MINIFLOAT), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
])
def test_append_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _append(**kwargs)
    assert rc == want, (case, rc, msg)
    assert ("KV cache" in msg or "quantizer" in msg) and len(msg) > 20, (case, msg)


def _attend(q=0x10000, cache=0x100000, cache_bytes=1 << 24, capacity=64, out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=1, heads=4, kv=4, S=1, T=40,
            D=64, fmts=None, mask=None, causal=0, dtype=_lib.F16):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    rc = L.lqer_attention_q_decode_kv(q, cache, cache_bytes, capacity, mask, out, None, dtype, batch, heads, kv, S, T, D, tri(heads * S * D, S * D, D),
                                      tri(0, 0, T) if mask else None, tri(heads * S * D, S * D, D), 0.125, causal, C.byref(fmts[0]), C.byref(fmts[1]),
                                      C.byref(fmts[2]), C.byref(fmts[3]), ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("S = 9", dict(S=9), E_UNSUPPORTED),
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("null q", dict(q=None), E_INVALID),
    ("null cache", dict(cache=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("cache not 16-byte aligned", dict(cache=0x100008), E_INVALID),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("short workspace", dict(ws_bytes=_lib.lib().lqer_attention_q_decode_workspace_bytes(1, 4, 4, 1, 40, 64) - 1), E_INVALID),
    ("short cache", dict(cache_bytes=_layout_sum(2, 1, 4, 64, 64) - 1), E_INVALID),
    ("T > capacity", dict(T=65), E_INVALID),
    ("negative T", dict(T=-1), E_INVALID),
    ("mask and causal", dict(mask=0x60000, causal=1), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
])
def test_attention_refusals_before_any_gpu_call(case, kwargs, want):
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)


def test_workspace_bytes_are_the_decode_kernels():
    L = _lib.lib()
    for args in [(1, 32, 32, 1, 2048, 128), (2, 4, 2, 5, 37, 80), (0, 8, 2, 1, 300, 64)]:
        assert L.lqer_attention_q_decode_kv_workspace_bytes(*args) == L.lqer_attention_q_decode_workspace_bytes(*args)


def test_unpack_refusals():
    L = _lib.lib()
    f = _fmt()
    call = lambda cache=0x100000, T=40, D=64, kf=0x70000, fmt=f: L.lqer_kv_cache_unpack(cache, 1 << 24, _lib.F16, 1, 4, 64, D, T, C.byref(fmt),
                                                                                       C.byref(f), kf, None, None)
    assert call(cache=None) == E_INVALID and "KV cache" in L.lqer_last_error().decode()
    assert call(T=65) == E_INVALID
    assert call(kf=None) == E_INVALID
    assert call(D=40) == E_UNSUPPORTED
    assert call(fmt=_fmt(32)) == E_UNSUPPORTED


def test_covers():
    from lqer_amd import QuantizedKVCache

    assert QuantizedKVCache.covers(CFG, CFG, 128, torch.float16)
    assert all(QuantizedKVCache.covers(CFG, CFG, d, dt) for d in (16, 48, 128) for dt in (torch.float16, torch.bfloat16, torch.float32))
    mini = json.loads(json.dumps(CFG))
    mini["w_quantizer"] = {"name": "minifloat", "width": 8, "exponent_width": 4, "exponent_bias": None}
    b32 = json.loads(json.dumps(CFG))
    b32["w_quantizer"]["block_size"] = [1, 32]
    refused = [(mini, CFG, 64, torch.float16), (CFG, mini, 64, torch.float16), (b32, CFG, 64, torch.float16), (CFG, b32, 64, torch.float16),
               (CFG, CFG, 160, torch.float16), (CFG, CFG, 24, torch.float16), (CFG, CFG, 64, torch.float64)]
    for cfg0, cfg1, d, dt in refused:
        assert not QuantizedKVCache.covers(cfg0, cfg1, d, dt)
        with pytest.raises(NotImplementedError):  # (raised before any allocation: no device is needed)
            QuantizedKVCache(1, 2, d, cfg0, cfg1, dt, "cuda:0")


def test_public_names():
    import lqer_amd
    from lqer_amd.attention import quantized_kv_cache  # noqa: F401

    assert "QuantizedKVCache" in lqer_amd.__all__ and "attention_flexible_cached" in lqer_amd.__all__

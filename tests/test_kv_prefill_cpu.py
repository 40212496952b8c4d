"""The prefill kernel over the packed KV cache (lqer_attention_q_kv; csrc/kv_cache.hip's image kernels, csrc/attn_q.hip), the part that
needs no GPU: the two C-ABI exports are declared, exported and bound with lqer_attention_q_decode_kv's argument list, the workspace is
lqer_attention_q's, every refusal comes with its code and a message before anything touches the device - and more than 8 query rows
are not one of them -, and the Python side takes the new keywords."""
import ctypes as C
import inspect
import os
import re

import pytest

from lqer_amd import _lib
from test_kv_cache_cpu import E_INVALID, E_UNSUPPORTED, MINIFLOAT, _fmt, _layout_sum, tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lqer_attention_q_kv_workspace_bytes", "lqer_attention_q_kv")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    assert "#define LQER_ABI_VERSION 14" in hdr
    assert _lib.SIGNATURES["lqer_attention_q_kv"] == _lib.SIGNATURES["lqer_attention_q_decode_kv"]
    # ... which is lqer_attention_q's with (k, v) -> (cache, cache_bytes, capacity) and without their two stride arrays
    raw, kv = _lib.SIGNATURES["lqer_attention_q"][1], _lib.SIGNATURES["lqer_attention_q_kv"][1]
    assert kv == raw[:1] + [C.c_void_p, C.c_size_t, C.c_int64] + raw[3:14] + raw[16:]
    assert _lib.SIGNATURES["lqer_attention_q_kv_workspace_bytes"] == _lib.SIGNATURES["lqer_attention_q_workspace_bytes"]


def test_workspace_bytes_are_the_prefill_kernels():
    L = _lib.lib()
    for args in [(1, 32, 32, 512, 4096, 128), (2, 4, 2, 40, 77, 80), (0, 8, 2, 9, 300, 64)]:
        assert L.lqer_attention_q_kv_workspace_bytes(*args) == L.lqer_attention_q_workspace_bytes(*args)
    # [K image: Z x Tp x Dp bf16][V image: Z x 128 x Tv bf16]
    assert L.lqer_attention_q_kv_workspace_bytes(2, 4, 2, 40, 77, 80) == 4 * 128 * 128 * 2 + 4 * 128 * 128 * 2
    assert L.lqer_attention_q_kv_workspace_bytes(0, 8, 2, 9, 300, 64) == 0


def _ws_bytes(batch=1, heads=4, kv=4, S=12, T=40, D=64):
    return _lib.lib().lqer_attention_q_workspace_bytes(batch, heads, kv, S, T, D)


def _attend(q=0x10000, cache=0x100000, cache_bytes=1 << 24, capacity=64, out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=1, heads=4, kv=4, S=12,
            T=40, D=64, fmts=None, mask=None, causal=0, dtype=_lib.F16, q_strides=True, out_strides=True, mask_strides=True):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    fp = [C.byref(f) if f is not None else None for f in fmts]
    rc = L.lqer_attention_q_kv(q, cache, cache_bytes, capacity, mask, out, None, dtype, batch, heads, kv, S, T, D,
                               tri(heads * S * D, S * D, D) if q_strides else None, tri(0, 0, T) if mask and mask_strides else None,
                               tri(heads * S * D, S * D, D) if out_strides else None, 0.125, causal, fp[0], fp[1], fp[2], fp[3], ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    # lqer_attention_q's
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("Q width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("K minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), E_UNSUPPORTED),
    ("V block 32", dict(fmts=[_fmt(), _fmt(), _fmt(), _fmt(32)]), E_UNSUPPORTED),
    ("null format", dict(fmts=[_fmt(), _fmt(), None, _fmt()]), E_INVALID),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("null q", dict(q=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("null q strides", dict(q_strides=False), E_INVALID),
    ("null out strides", dict(out_strides=False), E_INVALID),
    ("null mask strides", dict(mask=0x60000, mask_strides=False), E_INVALID),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("mask and causal", dict(mask=0x60000, causal=1), E_INVALID),
    ("short workspace", dict(ws_bytes=_ws_bytes() - 1), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("T beyond the image grid", dict(T=65535 * 64 + 1, capacity=1 << 23, cache_bytes=1 << 40, ws_bytes=1 << 40), E_UNSUPPORTED),
    ("negative S", dict(S=-1), E_INVALID),
    ("negative T", dict(T=-1), E_INVALID),
    ("T = 0", dict(T=0), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    # the cache's (kv_cache_check)
    ("null cache", dict(cache=None), E_INVALID),
    ("cache not 16-byte aligned", dict(cache=0x100008), E_INVALID),
    ("short cache", dict(cache_bytes=_layout_sum(2, 1, 4, 64, 64) - 1), E_INVALID),
    ("T > capacity", dict(T=65), E_INVALID),
    ("capacity = 0", dict(capacity=0), E_INVALID),
    # more than 8 query rows are taken: these get as far as the workspace check, the last one made (nothing is launched)
    ("S = 9, short workspace", dict(S=9, ws_bytes=_ws_bytes(S=9) - 1), E_INVALID),
    ("S = 1000, short workspace", dict(S=1000, ws_bytes=_ws_bytes(S=1000) - 1), E_INVALID),
    ("S = 1000, short cache", dict(S=1000, cache_bytes=_layout_sum(2, 1, 4, 64, 64) - 1), E_INVALID),
])
def test_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)
    if case.startswith("S = "):
        assert ("workspace" in msg or "KV cache of" in msg) and "query rows" not in msg, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith("attention_q_kv:"), (case, msg)  # the message names the call


def test_nothing_to_do_is_ok():
    assert _attend(batch=0)[0] == 0 and _attend(S=0)[0] == 0


def test_python_keywords():
    import lqer_amd
    from lqer_amd import attention_flexible_cached, kvcache
    from lqer_amd.attention import quantized_kv_cache

    for bad in ("flash", "unfused", ""):
        with pytest.raises(ValueError, match="kernel"):  # (checked first: no cache, no device needed)
            attention_flexible_cached(None, None, 0.125, kernel=bad)
    assert inspect.signature(attention_flexible_cached).parameters["kernel"].default is None
    p = inspect.signature(quantized_kv_cache).parameters
    assert p["chunked_prefill"].default is False and p["capacity"].default == 256
    assert callable(kvcache.prefill_packed) and callable(kvcache.attend_packed)
    assert inspect.signature(kvcache.prefill_packed) == inspect.signature(kvcache.attend_packed)
    assert lqer_amd.__all__ == ["LinearFlexible", "LinearFlexibleLqer", "get_quantized_layer_cls", "matmul_flexible", "bmm_flexible",
                                "attention_flexible", "get_quantized_func", "QuantizedKVCache", "attention_flexible_cached"]


def test_layer_option_reaches_the_layers():
    """The cache layer keeps the option (quantized_kv_cache hands it over positionally, after the capacity)."""
    from lqer_amd import attention as A

    cls = A._kv_layer_cls()
    assert cls({}, {}).chunked_prefill is False and cls({}, {}, 64, True).chunked_prefill is True

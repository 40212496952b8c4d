"""The prefill kernel over the paged KV pool (lqer_attention_q_paged; csrc/kv_cache.hip's paged image kernels, csrc/attn_q.hip's
per-sequence-length instantiation), the part that needs no GPU: the two C-ABI exports are declared, exported and bound with
lqer_attention_q_decode_paged's argument list, the workspace is lqer_attention_q_kv's at T = max_len, every refusal comes with its
code and a message before anything touches the device - more than 8 query rows are not one of them - and attention_flexible_paged
takes the `kernel` keyword."""
import ctypes as C
import inspect
import os
import re

import pytest

from lqer_amd import _lib
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, MINIFLOAT, POOL_OK, _fmt, tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lqer_attention_q_paged_workspace_bytes", "lqer_attention_q_paged")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    assert "#define LQER_ABI_VERSION 14" in hdr
    assert _lib.SIGNATURES["lqer_attention_q_paged"] == _lib.SIGNATURES["lqer_attention_q_decode_paged"]  # word for word
    assert _lib.SIGNATURES["lqer_attention_q_paged_workspace_bytes"] == _lib.SIGNATURES["lqer_attention_q_decode_paged_workspace_bytes"]


def test_workspace_bytes_are_the_prefill_kernels_at_max_len():
    L = _lib.lib()
    for args in [(4, 32, 32, 128, 2048, 128), (5, 4, 2, 20, 48, 48), (4, 8, 2, 200, 304, 64), (3, 2, 1, 33, 2064, 16), (1, 32, 32, 512, 4096, 128),
                 (2, 4, 2, 1, 1, 16)]:
        assert L.lqer_attention_q_paged_workspace_bytes(*args) == L.lqer_attention_q_kv_workspace_bytes(*args) > 0
    # [K image: Z x Tp x Dp bf16][V image: Z x 128 x Tv bf16], Tp = max_len up to 128, Dp = D up to 64, Tv = max_len up to 64
    assert L.lqer_attention_q_paged_workspace_bytes(5, 4, 2, 20, 48, 48) == 10 * 128 * 64 * 2 + 10 * 128 * 64 * 2
    assert L.lqer_attention_q_paged_workspace_bytes(4, 8, 2, 200, 304, 64) == 8 * 384 * 64 * 2 + 8 * 128 * 320 * 2
    for zero in [(0, 8, 2, 9, 300, 64), (2, 8, 2, 9, 0, 64), (2, 8, 2, 9, -1, 64), (2, 0, 2, 9, 300, 64), (2, 8, 2, 9, 300, 0)]:  # 0 where that function is
        assert L.lqer_attention_q_paged_workspace_bytes(*zero) == L.lqer_attention_q_kv_workspace_bytes(*zero) == 0


def _ws_bytes(batch=2, heads=4, kv=4, S=12, max_len=64, D=64):
    return _lib.lib().lqer_attention_q_paged_workspace_bytes(batch, heads, kv, S, max_len, D)


def _attend(q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
            out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=2, heads=4, kv=4, S=12, D=64, fmts=None, causal=0, dtype=_lib.F16, qs=True, os_=True):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = tri(heads * S * D, S * D, D)
    rc = L.lqer_attention_q_paged(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, dtype, batch, heads, kv,
                                  S, D, st if qs else None, st if os_ else None, 0.125, causal,
                                  *[C.byref(f) if f != "null" else None for f in fmts], ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    # what lqer_attention_q_kv refuses and still applies
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("Q width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("K minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), E_UNSUPPORTED),
    ("V block 32", dict(fmts=[_fmt(), _fmt(), _fmt(), _fmt(32)]), E_UNSUPPORTED),
    ("null format", dict(fmts=[_fmt(), "null", _fmt(), _fmt()]), E_INVALID),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("negative batch", dict(batch=-1), E_INVALID),
    ("negative S", dict(S=-1), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    ("null q", dict(q=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null q strides", dict(qs=False), E_INVALID),
    ("null out strides", dict(os_=False), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("short workspace", dict(ws_bytes=_ws_bytes() - 1), E_INVALID),
    ("S beyond the launch grid", dict(S=(1 << 30) + 1), E_UNSUPPORTED),
    ("max_len beyond the image grid", dict(max_len=65535 * 64 + 1, stride=1 << 19, ws_bytes=1 << 40), E_UNSUPPORTED),
    ("batch > 65535", dict(batch=65536), E_UNSUPPORTED),
    ("kv_heads > 65535", dict(heads=65536, kv=65536, batch=1), E_UNSUPPORTED),
    ("batch x kv_heads > 65535", dict(batch=16384, ws_bytes=1 << 40), E_UNSUPPORTED),
    # the pool's and the metadata's (lqer_attention_q_decode_paged's)
    ("null block_table", dict(tbl=None), E_INVALID),
    ("null seq_slots", dict(seq_slots=None), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("pages = 0", dict(pages=0), E_INVALID),
    ("slots = 0", dict(slots=0), E_INVALID),
    ("table_stride = 0", dict(stride=0), E_INVALID),
    ("max_len = 0", dict(max_len=0), E_INVALID),
    ("negative max_len", dict(max_len=-1), E_INVALID),
    ("max_len > 16 table_stride", dict(max_len=65), E_INVALID),
    ("max_len > 2^30", dict(max_len=(1 << 30) + 1, stride=1 << 27, ws_bytes=1 << 62), E_UNSUPPORTED),
    ("null pool", dict(pool=None), E_INVALID),
    ("pool not 16-byte aligned", dict(pool=0x100008), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
    # more than 8 query rows are taken: these get as far as the last checks made (nothing is launched)
    ("S = 9, short workspace", dict(S=9, ws_bytes=_ws_bytes(S=9) - 1), E_INVALID),
    ("S = 300, short workspace", dict(S=300, ws_bytes=_ws_bytes(S=300) - 1), E_INVALID),
    ("S = 9, short pool", dict(S=9, pool_bytes=POOL_OK - 1), E_INVALID),
    ("S = 300, short pool", dict(S=300, pool_bytes=POOL_OK - 1), E_INVALID),
])
def test_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)
    if case.startswith("S = "):
        assert ("workspace" in msg or "KV pool of" in msg) and "query rows" not in msg, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith("attention_q_paged:"), (case, msg)  # the message names the call


def test_nothing_to_do_is_ok():
    assert _attend(batch=0)[0] == 0 and _attend(S=0)[0] == 0


def test_python_keyword():
    import lqer_amd
    from lqer_amd import attention_flexible_paged

    p = inspect.signature(attention_flexible_paged).parameters
    assert p["kernel"].default == "decode"
    assert list(p)[:8] == ["q", "cache", "seqs", "scaling", "causal", "out_layout", "return_stats", "ws"]  # the earlier parameters, in place
    for bad in ("flash", "unfused", "", None):
        with pytest.raises(ValueError, match="kernel"):  # (checked first: no cache, no device needed)
            attention_flexible_paged(None, None, [], 0.125, kernel=bad)
    assert "attention_flexible_paged" not in lqer_amd.__all__ and callable(lqer_amd.attention_flexible_paged)

"""Per-sequence query counts on the split decode kernels of the paged KV pool (lqer_attention_q_decode_paged_ragged; the ragged
instantiation of csrc/attn_decode.hip's three kernels; attention_flexible_paged_decode_ragged, attention_flexible_paged_ragged's one
decode call and its .plan), the part that needs no GPU: the two C-ABI exports are declared, exported and bound, the workspace follows
the packed tokens, every refusal comes with its code and a message before anything touches the device, the plan of a step names its
library calls from host arithmetic, and the Python side refuses what it must before a launch."""
import ctypes as C
import inspect
import os
import re

import pytest

from lqer_amd import _lib
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, MINIFLOAT, POOL_OK, _fmt
from test_kv_ragged_cpu import _host_cache, _step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lqer_attention_q_decode_paged_ragged_workspace_bytes", "lqer_attention_q_decode_paged_ragged")
DECODE, PREFILL = "lqer_attention_q_decode_paged_ragged", "lqer_attention_q_paged_ragged"
pair = lambda a, b: (C.c_int64 * 2)(a, b)


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    assert "#define LQER_ABI_VERSION 14" in hdr
    i64 = C.c_int64
    # lqer_attention_q_paged_ragged's list plus one int64: the window
    assert _lib.SIGNATURES[DECODE] == (_lib.SIGNATURES[PREFILL][0], _lib.SIGNATURES[PREFILL][1] + [i64])
    assert _lib.SIGNATURES[NEW[0]] == (C.c_size_t, [i64] * 4)  # (total, heads, max_len, D)


def test_workspace_bytes_follow_the_packed_tokens():
    L = _lib.lib()
    ws, uniform = L.lqer_attention_q_decode_paged_ragged_workspace_bytes, L.lqer_attention_q_decode_paged_workspace_bytes
    up = lambda v: (v + 255) // 256 * 256
    for total, heads, max_len, D in [(36, 16, 2176, 128), (1, 4, 16, 48), (17, 8, 304, 64), (71, 32, 4224, 128), (64, 2, 1, 16), (9, 4, 257, 48)]:
        got = ws(total, heads, max_len, D)
        # the three parts of the uniform call, rows = total heads: the same size as that call at batch 1, S = total, whatever kv_heads is
        for kv in (1, 2, heads):
            if heads % kv == 0:
                assert got == uniform(1, heads, kv, total, max_len, D) > 0
        rows, tp = total * heads, (max_len + 127) // 128 * 128
        nchs = (max_len + 15) // 16 if max_len <= 256 else (16 if max_len <= 2048 else (max_len + 127) // 128)
        assert got == up(rows * tp * 4) + up(rows * nchs * 2 * 4) + up(rows * nchs * D * 4)
    # total x heads, max_len and D only: 15 one-token decoders and one 8-row sequence cost 23 tokens, not 16 x 8
    assert ws(23, 32, 4224, 128) < uniform(16, 32, 8, 8, 4224, 128) and ws(23, 32, 4224, 128) == uniform(23, 32, 8, 1, 4224, 128)
    for zero in [(0, 8, 300, 64), (-1, 8, 300, 64), (9, 0, 300, 64), (9, 8, 0, 64), (9, 8, -1, 64), (9, 8, 300, 0)]:
        assert ws(*zero) == 0


def _ws_bytes(total=13, heads=4, max_len=64, D=64):
    return _lib.lib().lqer_attention_q_decode_paged_ragged_workspace_bytes(total, heads, max_len, D)


def _attend(q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
            out=0x40000, ws=0x50000, ws_bytes=1 << 22, batch=2, heads=4, kv=4, starts=0x500000, max_s=8, total=13, D=64, fmts=None, causal=0,
            dtype=_lib.F16, qs=True, os_=True, window=0):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = pair(heads * D, D)
    rc = L.lqer_attention_q_decode_paged_ragged(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, dtype, batch,
                                                heads, kv, starts, max_s, total, D, st if qs else None, st if os_ else None, 0.125, causal,
                                                *[C.byref(f) if f != "null" else None for f in fmts], ws, ws_bytes, None, window)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    # the additions
    ("null q_starts", dict(starts=None), E_INVALID),
    ("max_s = 0", dict(max_s=0), E_INVALID),
    ("negative max_s", dict(max_s=-1), E_INVALID),
    ("max_s = 9", dict(max_s=9), E_INVALID),
    ("max_s = 300", dict(max_s=300), E_INVALID),
    ("negative total", dict(total=-1), E_INVALID),
    ("negative window", dict(window=-1, causal=1), E_INVALID),
    ("a window without causal", dict(window=8, causal=0), E_INVALID),
    ("short workspace", dict(ws_bytes=_ws_bytes() - 1), E_INVALID),
    ("short workspace with a window", dict(ws_bytes=_ws_bytes() - 1, window=8, causal=1), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    # what lqer_attention_q_decode_paged refuses
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("Q width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("K minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), E_UNSUPPORTED),
    ("V block 32", dict(fmts=[_fmt(), _fmt(), _fmt(), _fmt(32)]), E_UNSUPPORTED),
    ("null format", dict(fmts=[_fmt(), "null", _fmt(), _fmt()]), E_INVALID),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("negative batch", dict(batch=-1), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    ("null q", dict(q=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null q strides", dict(qs=False), E_INVALID),
    ("null out strides", dict(os_=False), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("batch > 65535", dict(batch=65536), E_UNSUPPORTED),
    ("kv_heads > 65535", dict(heads=65536, kv=65536, batch=1), E_UNSUPPORTED),
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
    # a bound of one row, a window of one key: these get as far as the last checks made (nothing is launched)
    ("max_s = 1, short workspace", dict(max_s=1, ws_bytes=_ws_bytes() - 1), E_INVALID),
    ("window = 1, short pool", dict(window=1, causal=1, pool_bytes=POOL_OK - 1), E_INVALID),
])
def test_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith("attention_q_decode_paged_ragged:"), (case, msg)  # the message names the call
    if case.startswith("short workspace"):
        assert "lqer_attention_q_decode_paged_ragged_workspace_bytes" in msg, msg


def test_nothing_to_do_is_ok():
    assert _attend(batch=0)[0] == 0 and _attend(total=0)[0] == 0
    assert _attend(batch=0, window=4, causal=1)[0] == 0 and _attend(total=0, window=4, causal=1)[0] == 0


# ---- the plan of a step: which library calls, from host arithmetic alone ----------------------------------------------------------------
def _plan(counts, cache=None, **kw):
    from lqer_amd import attention_flexible_paged_ragged

    cache = cache or _host_cache(4, 8, None, max_pages_per_seq=4)
    return attention_flexible_paged_ragged.plan(cache, list(range(len(counts))), counts, **kw)


def test_plan():
    # a verify step with every count of 1 .. 8: ONE decode call on a view of q (one call per distinct count made eight)
    assert _plan((1, 2, 3, 4, 5, 6, 7, 8)) == [{"call": DECODE, "seqs": list(range(8)), "rows": "view", "window": None}]
    # a prompt chunk between the decoders: their rows are gathered once; the chunk's own rows are one range
    assert _plan((1, 1, 33, 1)) == [{"call": DECODE, "seqs": [0, 1, 3], "rows": "gathered", "window": None},
                                    {"call": PREFILL, "seqs": [2], "rows": "view", "window": None}]
    # the decoders in front, the chunks behind: two views; a count of 0 is in no call
    assert _plan((1, 8, 0, 9, 200)) == [{"call": DECODE, "seqs": [0, 1], "rows": "view", "window": None},
                                        {"call": PREFILL, "seqs": [3, 4], "rows": "view", "window": None}]
    assert _plan((9, 1, 33)) == [{"call": DECODE, "seqs": [1], "rows": "view", "window": None},
                                 {"call": PREFILL, "seqs": [0, 2], "rows": "gathered", "window": None}]
    assert _plan((0, 0)) == [] and _plan(()) == []
    # kernel="prefill" is what it was: the whole batch in one call of the prefill kernel
    assert _plan((1, 2, 3, 4, 5, 6, 7, 8), kernel="prefill") == [{"call": PREFILL, "seqs": list(range(8)), "rows": "view", "window": None}]
    assert _plan((1, 0, 33, 1), kernel="prefill") == [{"call": PREFILL, "seqs": [0, 2, 3], "rows": "view", "window": None}]
    # the window: the cache's by default, an explicit one instead; the decode call runs under it, the prefill kernel has no rule
    windowed = _host_cache(4, 8, 16, max_pages_per_seq=4)
    assert _plan((1, 12, 3), windowed) == [{"call": DECODE, "seqs": [0, 2], "rows": "gathered", "window": 16},
                                           {"call": PREFILL, "seqs": [1], "rows": "view", "window": None}]
    assert _plan((1, 3), windowed, window=5)[0]["window"] == 5 and _plan((1, 3), window=5)[0]["window"] == 5
    for bad in (dict(kernel="decode"), dict(kernel="flash"), dict(window=0), dict(window=2.5)):
        with pytest.raises(ValueError):
            _plan((1, 2), **bad)
    for counts in ((1, -1), "ab"):
        with pytest.raises(ValueError, match="counts"):
            _plan(counts)
    with pytest.raises(ValueError, match="counts"):
        from lqer_amd import attention_flexible_paged_ragged
        attention_flexible_paged_ragged.plan(windowed, [0, 1], [1])


# ---- what the Python side refuses, on a cache in host memory whose launches do nothing ----------------------------------------------------
def test_python_interface_and_refusals():
    import torch

    import lqer_amd
    from lqer_amd import attention_flexible_paged_decode_ragged, attention_flexible_paged_ragged

    p = inspect.signature(attention_flexible_paged_decode_ragged).parameters
    assert list(p) == ["q", "cache", "seqs", "counts", "scaling", "causal", "return_stats", "ws", "window"]
    assert p["causal"].default is False and p["return_stats"].default is False and p["ws"].default is None and p["window"].default is None
    assert list(inspect.signature(attention_flexible_paged_ragged.plan).parameters) == ["cache", "seqs", "counts", "kernel", "window"]
    assert inspect.signature(attention_flexible_paged_ragged.plan).parameters["kernel"].default == "auto"
    assert callable(lqer_amd.attention_flexible_paged_decode_ragged) and "attention_flexible_paged_decode_ragged" not in lqer_amd.__all__

    cache = _host_cache(8, 4, None, max_pages_per_seq=2)  # kv_heads 2, head_dim 16, fp16, on the host
    a, b, short, freed = (cache.alloc() for _ in range(4))
    _step(cache, [a, short], [30, 5])
    cache.free(freed)
    q = torch.zeros(9, 4, 16, dtype=torch.float16)
    books = lambda: (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:], cache.pt.pages_of[:])
    state = books()
    for what, qq, seqs, counts, kw, match in [
            ("a count of 9", q, [a], [9], {}, "up to 8"),
            ("a count of 9 beside others", torch.zeros(10, 4, 16, dtype=torch.float16), [short, a], [1, 9], dict(causal=True), "up to 8"),
            ("a window without causal", q, [a, short], [8, 1], dict(window=64), "causal"),
            ("a window of 0", q, [a, short], [8, 1], dict(window=0, causal=True), "window"),
            ("a window that is no int", q, [a, short], [8, 1], dict(window=2.5, causal=True), "window"),
            ("len(counts) != len(seqs)", q, [a, short], [8], {}, "one count >= 0 per sequence"),
            ("a negative count", q, [a, short], [8, -1], {}, "one count >= 0 per sequence"),
            ("counts that are no ints", q, [a, short], "ab", {}, "one count >= 0 per sequence"),
            ("sum(counts) != q.shape[0]", q, [a, short], [7, 1], {}, r"is not \[sum\(counts\)"),
            ("causal with counts[b] > length_b", q, [a, short], [3, 6], dict(causal=True), "causal needs 6 query rows"),
            ("an empty sequence with a count", q, [a, b], [8, 1], {}, "an empty sequence"),
            ("freed", q, [a, freed], [8, 1], {}, "unknown or already freed"),
            ("named twice", q, [a, a], [8, 1], {}, "named twice"),
            ("dtype", q.float(), [a, short], [8, 1], {}, "for a cache"),
            ("head count", q[:, :3], [a, short], [8, 1], {}, "for a cache"),
            ("head dim", q[..., :8], [a, short], [8, 1], {}, "for a cache"),
            ("q is not [total, h, d]", q.unsqueeze(0), [a, short], [8, 1], {}, r"is not \[sum\(counts\)")]:
        with pytest.raises(ValueError, match=match):
            attention_flexible_paged_decode_ragged(qq, cache, seqs, counts, 1.0, **kw)
            pytest.fail(what)
    assert books() == state
    # the messages name the function; the shared ones are attention_flexible_paged_ragged's wording under its own name
    with pytest.raises(ValueError, match=r"^attention_flexible_paged_decode_ragged: counts \[8, -1\] for 2 sequences"):
        attention_flexible_paged_decode_ragged(q, cache, [a, short], [8, -1], 1.0)
    with pytest.raises(ValueError, match=r"^attention_flexible_paged_ragged: counts \[8, -1\] for 2 sequences"):
        attention_flexible_paged_ragged(q, cache, [a, short], [8, -1], 1.0)
    # a released sequence and a window wider than the cache's: the keys are gone
    win = _host_cache(12, 2, 16, max_pages_per_seq=12)
    s = win.alloc()
    _step(win, [s], [40])
    _step(win, [s], [24])
    assert win.pt.released[win.pt.slot(s)] == 2
    with pytest.raises(ValueError, match="released"):
        attention_flexible_paged_decode_ragged(q[:2], win, [s], [2], 1.0, causal=True, window=17)
    with pytest.raises(ValueError, match="causal"):  # the cache's window is the default, and it needs the causal rule
        attention_flexible_paged_decode_ragged(q[:2], win, [s], [2], 1.0)
    # attention_flexible_paged_ragged keeps its kernel values: "decode" still raises there
    for bad in ("flash", "decode", "", None):
        with pytest.raises(ValueError, match="kernel"):
            attention_flexible_paged_ragged(None, None, [], [], 0.125, kernel=bad)

"""Per-sequence token counts on the paged KV pool (lqer_kv_pool_append_ragged, lqer_attention_q_paged_ragged; csrc/kv_cache.hip's and
csrc/attn_q.hip's ragged instantiations; PagedKVCache.append_ragged, attention_flexible_paged_ragged), the part that needs no GPU: the
three C-ABI exports are declared, exported and bound, the workspace is lqer_attention_q_paged's, every refusal comes with its code and
a message before anything touches the device, and the page allocator reserves, commits and - on a window - releases by one count per
sequence, all or nothing."""
import ctypes as C
import inspect
import os
import re

import pytest

from lqer_amd import _lib
from lqer_amd.kvcache import PageTable
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, MINIFLOAT, POOL_OK, _fmt, _state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lqer_kv_pool_append_ragged", "lqer_attention_q_paged_ragged_workspace_bytes", "lqer_attention_q_paged_ragged")
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
    vp, i64 = C.c_void_p, C.c_int64
    # lqer_kv_pool_append's list with new_starts and max_n in front of k_new, and `total` in n's place
    ap, rg = _lib.SIGNATURES["lqer_kv_pool_append"][1], _lib.SIGNATURES["lqer_kv_pool_append_ragged"][1]
    assert rg == ap[:9] + [vp, i64] + ap[9:]
    # lqer_attention_q_paged's list with S -> (q_starts, max_s, total)
    pg, rg = _lib.SIGNATURES["lqer_attention_q_paged"][1], _lib.SIGNATURES["lqer_attention_q_paged_ragged"][1]
    assert rg == pg[:16] + [vp, i64, i64] + pg[17:]
    assert _lib.SIGNATURES["lqer_attention_q_paged_ragged_workspace_bytes"] == _lib.SIGNATURES["lqer_attention_q_paged_workspace_bytes"]


def test_workspace_bytes_are_the_paged_prefill_calls():
    L = _lib.lib()
    for args in [(4, 32, 32, 128, 2048, 128), (5, 4, 2, 20, 48, 48), (4, 8, 2, 200, 304, 64), (3, 2, 1, 33, 2064, 16), (1, 32, 32, 512, 4096, 128),
                 (2, 4, 2, 1, 1, 16)]:
        assert L.lqer_attention_q_paged_ragged_workspace_bytes(*args) == L.lqer_attention_q_paged_workspace_bytes(*args) > 0
    for zero in [(0, 8, 2, 9, 300, 64), (2, 8, 2, 9, 0, 64), (2, 8, 2, 9, -1, 64), (2, 0, 2, 9, 300, 64), (2, 8, 2, 9, 300, 0)]:
        assert L.lqer_attention_q_paged_ragged_workspace_bytes(*zero) == L.lqer_attention_q_paged_workspace_bytes(*zero) == 0
    # the images only: nothing follows max_s
    assert L.lqer_attention_q_paged_ragged_workspace_bytes(4, 8, 2, 1, 304, 64) == L.lqer_attention_q_paged_ragged_workspace_bytes(4, 8, 2, 4096, 304, 64)


def _append(pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
            starts=0x500000, max_n=3, k=0x20000, v=0x30000, ks=True, vs=True, dtype=_lib.F16, batch=2, kv=4, D=64, total=4, k_fmt=None, v_fmt=None):
    L = _lib.lib()
    k_fmt, v_fmt = k_fmt or _fmt(), v_fmt or _fmt()
    st = pair(kv * D, D)
    rc = L.lqer_kv_pool_append_ragged(pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, starts, max_n, k, v,
                                      st if ks else None, st if vs else None, dtype, batch, kv, D, total,
                                      C.byref(k_fmt) if k_fmt != "null" else None, C.byref(v_fmt) if v_fmt != "null" else None, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    # the additions
    ("null new_starts", dict(starts=None), E_INVALID),
    ("max_n = 0", dict(max_n=0), E_INVALID),
    ("negative max_n", dict(max_n=-1), E_INVALID),
    ("max_n > max_len", dict(max_n=65), E_INVALID),
    ("negative total", dict(total=-1), E_INVALID),
    ("null k strides", dict(ks=False), E_INVALID),
    ("null v strides", dict(vs=False), E_INVALID),
    # lqer_kv_pool_append's
    ("negative batch", dict(batch=-1), E_INVALID),
    ("kv_heads = 0", dict(kv=0), E_INVALID),
    ("pages = 0", dict(pages=0), E_INVALID),
    ("slots = 0", dict(slots=0), E_INVALID),
    ("table_stride = 0", dict(stride=0), E_INVALID),
    ("max_len = 0", dict(max_len=0), E_INVALID),
    ("max_len > 16 table_stride", dict(max_len=65), E_INVALID),
    ("max_len > 2^30", dict(max_len=(1 << 30) + 1, stride=1 << 27), E_UNSUPPORTED),
    ("null block_table", dict(tbl=None), E_INVALID),
    ("null seq_slots", dict(seq_slots=None), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("null pool", dict(pool=None), E_INVALID),
    ("pool not 16-byte aligned", dict(pool=0x100008), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
    ("null k_new", dict(k=None), E_INVALID),
    ("null v_new", dict(v=None), E_INVALID),
    ("null k format", dict(k_fmt="null"), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    ("block 32", dict(k_fmt=_fmt(32)), E_UNSUPPORTED),
    ("V block 32", dict(v_fmt=_fmt(32)), E_UNSUPPORTED),
    ("width 12", dict(v_fmt=_fmt(width=12)), E_UNSUPPORTED),
    ("minifloat", dict(k_fmt=MINIFLOAT), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("beyond one launch grid", dict(batch=1 << 20, max_n=1 << 20, max_len=1 << 20, stride=1 << 16), E_UNSUPPORTED),
])
def test_append_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _append(**kwargs)
    assert rc == want, (case, rc, msg)
    assert ("KV pool" in msg or "KV cache" in msg or "quantizer" in msg) and len(msg) > 20, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith("kv_pool_append_ragged:"), (case, msg)  # the message names the call


def _ws_bytes(batch=2, heads=4, kv=4, max_s=12, max_len=64, D=64):
    return _lib.lib().lqer_attention_q_paged_ragged_workspace_bytes(batch, heads, kv, max_s, max_len, D)


def _attend(q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
            out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=2, heads=4, kv=4, starts=0x500000, max_s=12, total=13, D=64, fmts=None, causal=0,
            dtype=_lib.F16, qs=True, os_=True):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = pair(heads * D, D)
    rc = L.lqer_attention_q_paged_ragged(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, dtype, batch, heads, kv,
                                         starts, max_s, total, D, st if qs else None, st if os_ else None, 0.125, causal,
                                         *[C.byref(f) if f != "null" else None for f in fmts], ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    # the additions
    ("null q_starts", dict(starts=None), E_INVALID),
    ("max_s = 0", dict(max_s=0), E_INVALID),
    ("negative max_s", dict(max_s=-1), E_INVALID),
    ("negative total", dict(total=-1), E_INVALID),
    # what lqer_attention_q_paged refuses
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
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("short workspace", dict(ws_bytes=_ws_bytes() - 1), E_INVALID),
    ("max_s beyond the launch grid", dict(max_s=(1 << 30) + 1), E_UNSUPPORTED),
    ("max_len beyond the image grid", dict(max_len=65535 * 64 + 1, stride=1 << 19, ws_bytes=1 << 40), E_UNSUPPORTED),
    ("batch > 65535", dict(batch=65536), E_UNSUPPORTED),
    ("kv_heads > 65535", dict(heads=65536, kv=65536, batch=1), E_UNSUPPORTED),
    ("batch x kv_heads > 65535", dict(batch=16384, ws_bytes=1 << 40), E_UNSUPPORTED),
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
    # a bound of one row or of hundreds: these get as far as the last checks made (nothing is launched)
    ("max_s = 1, short workspace", dict(max_s=1, ws_bytes=_ws_bytes(max_s=1) - 1), E_INVALID),
    ("max_s = 300, short pool", dict(max_s=300, total=301, pool_bytes=POOL_OK - 1), E_INVALID),
])
def test_attention_refusals_before_any_gpu_call(case, kwargs, want):
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith("attention_q_paged_ragged:"), (case, msg)  # the message names the call
    if case == "short workspace":
        assert "lqer_attention_q_paged_ragged_workspace_bytes" in msg, msg


def test_nothing_to_do_is_ok():
    assert _attend(batch=0)[0] == 0 and _attend(total=0)[0] == 0
    assert _append(batch=0)[0] == 0 and _append(total=0)[0] == 0


# ---- the allocator with one count per sequence ----------------------------------------------------------------------------------------
def test_reserve_with_per_sequence_counts():
    pt = PageTable(num_pages=12, max_seqs=4, max_pages_per_seq=4)
    a, b, c, d = (pt.alloc() for _ in range(4))
    slots, before, taken = pt.reserve([a, b, c, d], [1, 17, 0, 48])
    assert before == [0, 0, 0, 0] and taken == [1, 2, 0, 3] and pt.pages_free == 6
    assert [pt.length(s) for s in (a, b, c, d)] == [0, 0, 0, 0]  # (the lengths advance once the launch is issued)
    pt.commit(slots, [1, 17, 0, 48])
    assert [pt.length(s) for s in (a, b, c, d)] == [1, 17, 0, 48] and pt.pages_of[pt.slot(c)] == 0
    used = [pt.table[pt.slot(s)][i] for s in (a, b, d) for i in range(pt.pages_of[pt.slot(s)])]
    assert len(set(used)) == 6
    # a count of 0 on a non-empty sequence takes none either - also at a page boundary; the others by their own counts
    slots, before, taken = pt.reserve([d, a, b], [0, 15, 16])  # 48 stays; 1 -> 16: the same page; 17 -> 33: one more
    assert before == [48, 1, 17] and taken == [0, 0, 1] and pt.pages_free == 5
    pt.commit(slots, [0, 15, 16])
    assert [pt.length(s) for s in (a, b, c, d)] == [16, 33, 0, 48]
    # all zero: nothing happens
    state = _state(pt)
    slots, before, taken = pt.reserve([a, c], [0, 0])
    assert taken == [0, 0]
    pt.commit(slots, [0, 0])
    assert _state(pt) == state
    # the int form is what it was
    slots, _, taken = pt.reserve([c], 5)
    assert taken == [1]
    pt.rollback(slots, taken)
    assert (pt.pages_free, pt.pages_of, pt.lengths) == (state[0], state[2], state[3])  # (the row keeps a stale entry beyond pages_of)


def test_reserve_with_counts_is_all_or_nothing():
    pt = PageTable(num_pages=5, max_seqs=3, max_pages_per_seq=3)
    a, b, c = pt.alloc(), pt.alloc(), pt.alloc()
    pt.commit(pt.reserve([a, b], [20, 20])[0], [20, 20])  # 2 + 2 pages, one left
    for what, seqs, n, exc in [("out of pages midway: the first fits, the second does not", [c, a], [16, 13], RuntimeError),
                               ("out of pages: the call needs two", [a, b, c], [13, 13, 0], RuntimeError),
                               ("beyond max_pages_per_seq", [c, a], [1, 29], RuntimeError),
                               ("a count too few", [a, b], [1], ValueError),
                               ("a count too many", [a], [1, 1], ValueError),
                               ("a negative count", [a, c], [1, -1], ValueError),
                               ("named twice", [c, c], [1, 0], ValueError),
                               ("unknown", [c, 7], [1, 1], KeyError),
                               ("n = 0 as an int", [c], 0, ValueError)]:
        before = _state(pt)
        with pytest.raises(exc):
            pt.reserve(seqs, n)
        assert _state(pt) == before, what
    # a full sequence with a count of 0 beside one that fits: taken
    pt2 = PageTable(num_pages=4, max_seqs=2, max_pages_per_seq=2)
    x, y = pt2.alloc(), pt2.alloc()
    pt2.commit(pt2.reserve([x], 32)[0], 32)
    slots, _, taken = pt2.reserve([x, y], [0, 32])
    assert taken == [0, 2] and pt2.pages_free == 0


def test_rollback_of_a_reservation_with_counts():
    pt = PageTable(num_pages=9, max_seqs=3, max_pages_per_seq=4)
    a, b, c = pt.alloc(), pt.alloc(), pt.alloc()
    pt.commit(pt.reserve([a, b], [20, 5])[0], [20, 5])
    owned = lambda: [pt.table[s][:pt.pages_of[s]] for s in range(3)]
    before = (pt.pages_free, owned(), pt.lengths[:])
    slots, _, taken = pt.reserve([b, c, a], [30, 0, 13])
    assert taken == [2, 0, 1] and pt.pages_free == 3
    got = owned()
    pt.rollback(slots, taken)
    assert (pt.pages_free, owned(), pt.lengths[:]) == before
    pt.reserve([b, c, a], [30, 0, 13])
    assert owned() == got


def _host_cache(num_pages, max_seqs, window, max_pages_per_seq):
    """A PagedKVCache whose buffers live in host memory and whose launches do nothing, or raise once `cache.refuse` is set: the
    bookkeeping of append() and append_ragged() runs as it is, and no device is needed or touched (test_kv_window_cpu.py's way)."""
    import json

    import torch

    from lqer_amd import PagedKVCache

    with open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")) as fh:
        cfg = json.load(fh)
    cache = PagedKVCache(num_pages, max_seqs, 2, 16, cfg, cfg, torch.float16, "cpu", max_pages_per_seq=max_pages_per_seq, window=window)
    cache.refuse = False

    def launch(*a):
        if cache.refuse:
            raise _lib.LqerHipError("the launch was refused")

    cache._launch_append = cache._launch_append_ragged = launch
    return cache


def _step(cache, seqs, counts):
    import torch

    kv = torch.zeros(sum(counts), 2, 16, dtype=torch.float16)
    cache.append_ragged(seqs, kv, kv, counts)


def test_window_release_with_per_sequence_counts_and_its_undo():
    """window = 16: a sequence gives up the pages wholly below min(T_after - W - 7, 16 (T_before // 16)) - by ITS count."""
    cache = _host_cache(12, 3, 16, max_pages_per_seq=12)
    pt = cache.pt
    a, b, c = cache.alloc(), cache.alloc(), cache.alloc()
    _step(cache, [a, b, c], [40, 40, 40])  # 3 pages each, nothing to release on an empty sequence
    assert [cache.pages_held(s) for s in (a, b, c)] == [3, 3, 3] and cache.pages_free == 3
    full = lambda: (pt.pages_free, pt._free_pages[:], pt.released[:], pt.pages_of[:], pt.lengths[:], pt._owners.copy().tolist(),
                    [pt.table[s][:pt.pages_of[s]] for s in range(3)])  # (beyond pages_of a row may keep a stale entry)
    before = full()
    # a: 1 key -> below min(41 - 23, 32) = 18: page 0 goes.  b: 24 keys -> below min(64 - 23, 32) = 32: pages 0 and 1.  c: 0 -> alone
    cache.refuse = True
    with pytest.raises(_lib.LqerHipError):
        _step(cache, [a, b, c], [1, 24, 0])
    assert full() == before  # the undo: the books, the free stack in its order
    cache.refuse = False
    with pytest.raises(RuntimeError):  # out of pages midway (b would need 9 more): released pages come back too
        _step(cache, [a, b, c], [1, 150, 0])
    assert full() == before
    _step(cache, [a, b, c], [1, 24, 0])
    assert [pt.released[pt.slot(s)] for s in (a, b, c)] == [1, 2, 0]
    assert [cache.length(s) for s in (a, b, c)] == [41, 64, 40] and [cache.pages_held(s) for s in (a, b, c)] == [2, 2, 3]
    assert cache.pages_free == 3 + 3 - 1  # three released, b's fourth page taken
    # the uniform append on the same sequences gives the same books: a count per sequence is that sequence's n
    import torch

    ref = _host_cache(12, 3, 16, max_pages_per_seq=12)
    ra, rb, rc = ref.alloc(), ref.alloc(), ref.alloc()
    kv = lambda batch, n: torch.zeros(batch, 2, n, 16, dtype=torch.float16)
    ref.append([ra, rb, rc], kv(3, 40), kv(3, 40))
    ref.append([ra], kv(1, 1), kv(1, 1)), ref.append([rb], kv(1, 24), kv(1, 24))
    assert (ref.pt.released, ref.pt.lengths, ref.pt.pages_of, ref.pages_free) == (pt.released, pt.lengths, pt.pages_of, pt.pages_free)
    # a cache without a window: counts of 0 and all-zero calls change nothing, a refusal rolls the reservation back
    plain = _host_cache(6, 2, None, max_pages_per_seq=3)
    x, y = plain.alloc(), plain.alloc()
    _step(plain, [x, y], [17, 0])
    assert (plain.length(x), plain.length(y), plain.pages_free) == (17, 0, 4)
    state = _state(plain.pt)
    _step(plain, [x, y], [0, 0])
    plain.refuse = True
    with pytest.raises(_lib.LqerHipError):
        _step(plain, [y, x], [20, 15])
    assert (plain.pages_free, plain.pt.pages_of, plain.pt.lengths) == (state[0], state[2], state[3])


def test_python_interface():
    import lqer_amd
    from lqer_amd import PagedKVCache, attention_flexible_paged_ragged

    p = inspect.signature(attention_flexible_paged_ragged).parameters
    assert list(p) == ["q", "cache", "seqs", "counts", "scaling", "causal", "return_stats", "ws", "kernel", "window"]
    assert p["kernel"].default == "auto" and p["causal"].default is False and p["window"].default is None
    assert list(inspect.signature(PagedKVCache.append_ragged).parameters) == ["self", "seqs", "k", "v", "counts"]
    for bad in ("flash", "decode", "", None):
        with pytest.raises(ValueError, match="kernel"):  # (checked first: no cache, no device needed)
            attention_flexible_paged_ragged(None, None, [], [], 0.125, kernel=bad)
    assert callable(lqer_amd.attention_flexible_paged_ragged) and "attention_flexible_paged_ragged" not in lqer_amd.__all__

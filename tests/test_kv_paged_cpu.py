"""The paged KV pool (csrc/kv_cache.hip, csrc/attn_decode.hip, csrc/kv_pack.h, lqer_amd/kvcache.py), the part that needs no GPU: the
five C-ABI exports are declared, exported and bound, the byte count follows the header's layout, the memory argument for paging is the
arithmetic the layout gives, every refusal comes with its code and a message before anything touches the device, and the page
allocator keeps its books - all or nothing - on the host."""
import ctypes as C
import os
import re

import pytest

from lqer_amd import _lib
from lqer_amd.kvcache import PAGE_KEYS, PageTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
NEW = ("lqer_kv_pool_bytes", "lqer_kv_pool_append", "lqer_kv_pool_gather", "lqer_attention_q_decode_paged_workspace_bytes",
       "lqer_attention_q_decode_paged")
DTS = ((_lib.F16, 2), (_lib.BF16, 2), (_lib.F32, 4))
up = lambda v: (v + 255) // 256 * 256


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    assert "#define LQER_ABI_VERSION 14" in hdr and "#define LQER_KV_PAGE_KEYS 16" in hdr and PAGE_KEYS == 16
    # lqer_attention_q_decode_kv's argument list with (cache, cache_bytes, capacity) -> (pool, pool_bytes, pages, slots, block_table,
    # table_stride, seq_slots, lens, max_len), without T, the mask and its strides
    kv, pg = _lib.SIGNATURES["lqer_attention_q_decode_kv"][1], _lib.SIGNATURES["lqer_attention_q_decode_paged"][1]
    vp, sz, i64 = C.c_void_p, C.c_size_t, C.c_int64
    assert pg == kv[:1] + [vp, sz, i64, i64, vp, i64, vp, vp, i64] + kv[5:12] + kv[13:15] + kv[16:]  # (kv[4] mask, kv[12] T, kv[15] mask strides)
    assert _lib.SIGNATURES["lqer_attention_q_decode_paged_workspace_bytes"] == _lib.SIGNATURES["lqer_attention_q_decode_workspace_bytes"]


def _layout_sum(esz, pages, slots, kv, D):
    """include/lqer_hip.h: K codes [pages][kv][16][D], K exponents [pages][kv][D], V codes [pages][kv][16][D], V exponents
    [pages][kv][D/16][16] (one byte each), K staging [slots][kv][16][D] of the dtype; each rounded up to 256 bytes."""
    items = pages * kv
    return up(items * 16 * D) + up(items * D) + up(items * 16 * D) + up(items * (D // 16) * 16) + up(slots * kv * 16 * D * esz)


def _dense_sum(esz, batch, kv, capacity, D):
    cap, z = (capacity + 15) // 16 * 16, batch * kv
    return up(z * cap * D) + up(z * (cap // 16) * D) + up(z * cap * D) + up(z * (cap // 16) * (D // 16) * 16) + up(z * 16 * D * esz)


def test_pool_bytes():
    L = _lib.lib()
    for dt, esz in DTS:
        for pages, slots, kv, D in [(1, 1, 1, 16), (7, 3, 2, 48), (4096, 64, 32, 128)]:
            assert L.lqer_kv_pool_bytes(dt, pages, slots, kv, D) == _layout_sum(esz, pages, slots, kv, D)
    for bad in [(_lib.F16, 4, 2, 2, 24), (_lib.F16, 4, 2, 2, 144), (7, 4, 2, 2, 64), (_lib.F16, 0, 2, 2, 64), (_lib.F16, 4, 0, 2, 64),
                (_lib.F16, 4, 2, 0, 64)]:
        assert L.lqer_kv_pool_bytes(*bad) == 0


def test_ragged_batch_pays_for_its_keys_not_for_its_longest_sequence():
    """The motivation's arithmetic: eight sequences of these lengths need sum(ceil(L / 16)) pages; the pool of exactly that many is
    smaller than the dense cache of batch 8 at capacity 2048 by the ratio of the pages in use to the pages the slab holds (the
    staging rows, one set per sequence on both sides, aside)."""
    L = _lib.lib()
    lens, kv, D = (64, 128, 256, 512, 1024, 1536, 2048, 2048), 32, 128
    pages = sum((n + 15) // 16 for n in lens)
    assert pages == sum(lens) // 16 == 476
    for dt, esz in DTS:
        pool, dense = L.lqer_kv_pool_bytes(dt, pages, len(lens), kv, D), L.lqer_kv_cache_bytes(dt, len(lens), kv, 2048, D)
        assert pool == _layout_sum(esz, pages, len(lens), kv, D) and dense == _dense_sum(esz, len(lens), kv, 2048, D)
        stage = len(lens) * kv * 16 * D * esz  # (a multiple of 256, like every section here: nothing is rounded)
        assert pool < dense
        assert (pool - stage) * (len(lens) * 2048 // 16) == (dense - stage) * pages  # codes and exponents: exactly pages / slab pages
        per_page = kv * (2 * 16 * D + 2 * D)
        assert dense - pool == (len(lens) * 2048 // 16 - pages) * per_page


def _fmt(block=16, width=8, kind=_lib.Q_MXINT):
    return _lib.QFmt(kind, width, block, 8, 127)


MINIFLOAT = _lib.QFmt(_lib.Q_MINIFLOAT, 8, 16, 4, 7)
tri = lambda a, b, c: (C.c_int64 * 3)(a, b, c)
POOL_OK = _layout_sum(2, 8, 4, 4, 64)  # pages 8, slots 4, kv 4, D 64, fp16


def _append(pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64, k=0x20000,
            v=0x30000, ks=True, vs=True, dtype=_lib.F16, batch=2, kv=4, D=64, n=3, k_fmt=None, v_fmt=None):
    L = _lib.lib()
    k_fmt, v_fmt = k_fmt or _fmt(), v_fmt or _fmt()
    st = tri(kv * n * D, n * D, D)
    rc = L.lqer_kv_pool_append(pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, k, v, st if ks else None, st if vs else None,
                               dtype, batch, kv, D, n, C.byref(k_fmt) if k_fmt != "null" else None, C.byref(v_fmt) if v_fmt != "null" else None,
                               None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("n = 0", dict(n=0), E_INVALID),
    ("negative n", dict(n=-1), E_INVALID),
    ("n > max_len", dict(n=65), E_INVALID),
    ("negative batch", dict(batch=-1), E_INVALID),
    ("kv_heads = 0", dict(kv=0), E_INVALID),
    ("pages = 0", dict(pages=0), E_INVALID),
    ("slots = 0", dict(slots=0), E_INVALID),
    ("table_stride = 0", dict(stride=0), E_INVALID),
    ("max_len = 0", dict(max_len=0), E_INVALID),
    ("max_len > 16 table_stride", dict(max_len=65), E_INVALID),
    ("max_len > 2^30", dict(max_len=(1 << 30) + 1, stride=1 << 27), E_UNSUPPORTED),  # (one code in every call: the attention's too)
    ("null block_table", dict(tbl=None), E_INVALID),
    ("null seq_slots", dict(seq_slots=None), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("null pool", dict(pool=None), E_INVALID),
    ("pool not 16-byte aligned", dict(pool=0x100008), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
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
    assert ("KV pool" in msg or "KV cache" in msg or "quantizer" in msg) and len(msg) > 20, (case, msg)


def _attend(q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
            out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=2, heads=4, kv=4, S=1, D=64, fmts=None, causal=0, dtype=_lib.F16, qs=True, os_=True):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = tri(heads * S * D, S * D, D)
    rc = L.lqer_attention_q_decode_paged(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, dtype, batch, heads, kv,
                                         S, D, st if qs else None, st if os_ else None, 0.125, causal,
                                         *[C.byref(f) if f != "null" else None for f in fmts], ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


WS_OK = _lib.lib().lqer_attention_q_decode_paged_workspace_bytes(2, 4, 4, 1, 64, 64)


@pytest.mark.parametrize("case, kwargs, want", [
    # what lqer_attention_q_decode_kv refuses and still applies
    ("S = 9", dict(S=9), E_UNSUPPORTED),
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("batch > 65535", dict(batch=65536), E_UNSUPPORTED),
    ("null q", dict(q=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null q strides", dict(qs=False), E_INVALID),
    ("null out strides", dict(os_=False), E_INVALID),
    ("null format", dict(fmts=[_fmt(), "null", _fmt(), _fmt()]), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("short workspace", dict(ws_bytes=WS_OK - 1), E_INVALID),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("negative batch", dict(batch=-1), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    # the pool's
    ("null block_table", dict(tbl=None), E_INVALID),
    ("null seq_slots", dict(seq_slots=None), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("pages = 0", dict(pages=0), E_INVALID),
    ("slots = 0", dict(slots=0), E_INVALID),
    ("table_stride = 0", dict(stride=0), E_INVALID),
    ("max_len = 0", dict(max_len=0), E_INVALID),
    ("negative max_len", dict(max_len=-1), E_INVALID),
    ("max_len > 16 table_stride", dict(max_len=65), E_INVALID),
    ("null pool", dict(pool=None), E_INVALID),
    ("pool not 16-byte aligned", dict(pool=0x100008), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
])
def test_attention_refusals_before_any_gpu_call(case, kwargs, want):
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)


def test_max_len_beyond_2_to_30_is_refused():
    rc, msg = _attend(max_len=(1 << 30) + 1, stride=1 << 27, ws_bytes=1 << 62)
    assert rc == E_UNSUPPORTED and "2^30" in msg, (rc, msg)


def _nch(T):
    c = 16 * min(max((T + 255) // 256, 1), 8)
    return c, (T + c - 1) // c


def test_workspace_strides_follow_max_len():
    """rows x (max_len rounded up to 128) scores, rows x nchs x (2 + D) statistics and partials, nchs the largest chunk count of ANY
    T <= max_len - not of max_len itself: 256 keys make 16 chunks, 257 make 9."""
    L = _lib.lib()
    assert [_nch(T)[1] for T in (255, 256, 257, 300, 2048, 2049)] == [16, 16, 9, 10, 16, 17]
    for batch, heads, S, max_len, D in [(2, 4, 1, 64, 64), (4, 8, 3, 304, 64), (3, 2, 8, 2064, 16), (1, 32, 1, 2048, 128), (2, 4, 2, 16, 48),
                                        (1, 2, 1, 5000, 32)]:
        rows, tp = batch * heads * S, (max_len + 127) // 128 * 128
        nchs = max(_nch(T)[1] for T in range(1, max_len + 1))
        assert all(_nch(T)[0] * _nch(T)[1] <= tp for T in range(1, max_len + 1))  # every sequence's padded scores fit a row
        assert L.lqer_attention_q_decode_paged_workspace_bytes(batch, heads, heads, S, max_len, D) == \
            up(rows * tp * 4) + up(rows * nchs * 2 * 4) + up(rows * nchs * D * 4)
    assert L.lqer_attention_q_decode_paged_workspace_bytes(0, 4, 4, 1, 64, 64) == 0
    assert L.lqer_attention_q_decode_paged_workspace_bytes(1, 4, 4, 1, 0, 64) == 0


def test_gather_refusals():
    L = _lib.lib()
    dense_ok = _dense_sum(2, 1, 4, 64, 64)

    def call(pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, D=64, tbl=0x200000, stride=4, slot=1, T=40, cache=0x500000, cache_bytes=1 << 24,
             capacity=64, dtype=_lib.F16):
        rc = L.lqer_kv_pool_gather(pool, pool_bytes, dtype, pages, slots, 4, D, tbl, stride, slot, T, cache, cache_bytes, capacity, None)
        msg = L.lqer_last_error().decode()
        assert rc == 0 or ("KV pool" in msg or "KV cache" in msg) and len(msg) > 20, msg
        return rc

    for kwargs in [dict(pool=None), dict(pool=0x100008), dict(pool_bytes=POOL_OK - 1), dict(tbl=None), dict(slot=4), dict(slot=-1), dict(T=65),
                   dict(T=-1), dict(T=40, capacity=32), dict(cache=None), dict(cache=0x500008), dict(cache_bytes=dense_ok - 1), dict(pages=0),
                   dict(stride=0), dict(T=64, capacity=64, stride=3), dict(dtype=9)]:
        assert call(**kwargs) == E_INVALID, kwargs
    assert call(D=40) == E_UNSUPPORTED


# ---- the allocator and the host mirror ---------------------------------------------------------------------------------------------
def _state(pt):
    return pt.pages_free, [row[:] for row in pt.table], pt.pages_of[:], pt.lengths[:]


def test_allocator_bookkeeping_and_reuse():
    pt = PageTable(num_pages=10, max_seqs=3, max_pages_per_seq=6)
    assert pt.pages_free == 10 and pt.max_len == 96
    a, b, c = pt.alloc(), pt.alloc(), pt.alloc()
    assert (a, b, c) == (0, 1, 2) and len({pt.slot(s) for s in (a, b, c)}) == 3
    with pytest.raises(RuntimeError):
        pt.alloc()  # no slot left
    slots, before, taken = pt.reserve([c, a], 17)  # two pages each, in the call's order
    assert slots == [pt.slot(c), pt.slot(a)] and before == [0, 0] and taken == [2, 2]
    assert pt.length(a) == 0  # (the lengths advance once the launch is issued)
    pt.commit(slots, 17)
    assert pt.length(a) == pt.length(c) == 17 and pt.length(b) == 0 and pt.pages_free == 6
    used = [pt.table[s][i] for s in slots for i in range(2)]
    assert len(set(used)) == 4 and all(0 <= p < 10 for p in used)  # no page in two live sequences
    slots, before, taken = pt.reserve([a], 15)  # 17 -> 32 keys: still two pages
    assert before == [17] and taken == [0] and pt.pages_free == 6
    pt.commit(slots, 15)
    slots, before, taken = pt.reserve([a], 1)  # the 33rd key opens a third page
    assert taken == [1] and pt.pages_free == 5
    pt.commit(slots, 1)
    mine = pt.table[pt.slot(a)][:3]
    pt.free(a)
    assert pt.pages_free == 8
    d = pt.alloc()  # a new id, a's slot and - first - a's pages
    assert d == 3 and pt.length(d) == 0
    slots, _, _ = pt.reserve([d], 48)
    pt.commit(slots, 48)
    assert sorted(pt.table[pt.slot(d)][:3]) == sorted(mine) and pt.pages_free == 5
    live = [pt.table[pt.slot(s)][i] for s in (c, d) for i in range(pt.pages_of[pt.slot(s)])]
    assert len(set(live)) == len(live) == 5


def test_allocator_refuses_with_nothing_taken():
    pt = PageTable(num_pages=5, max_seqs=3, max_pages_per_seq=3)
    a, b, c = pt.alloc(), pt.alloc(), pt.alloc()
    pt.commit(pt.reserve([a, b], 20)[0], 20)  # 2 + 2 pages, one left
    for what, seqs, n, exc in [("out of pages: the call needs two", [a, b], 13, RuntimeError),
                               ("out of pages: the first fits, the second does not", [c, a], 16, RuntimeError),
                               ("beyond max_pages_per_seq", [c, a], 29, RuntimeError),
                               ("named twice", [c, c], 1, ValueError),
                               ("unknown", [c, 7], 1, KeyError),
                               ("n = 0", [c], 0, ValueError)]:
        before = _state(pt)
        with pytest.raises(exc):
            pt.reserve(seqs, n)
        assert _state(pt) == before, what
    pt.free(b)
    before = _state(pt)
    for fn in (lambda: pt.reserve([a, b], 1), lambda: pt.free(b), lambda: pt.length(b), lambda: pt.slots([b])):
        with pytest.raises(KeyError):  # freed: the id is never valid again, though its slot is reused
            fn()
    assert _state(pt) == before
    assert pt.alloc() == 3 and pt.pages_free == 3


def test_rollback_of_a_reservation_whose_launch_was_refused():
    """reserve() then rollback() leaves the books as they were - pages_free, the pages each sequence owns, the lengths - and the next
    reserve() takes the same pages."""
    pt = PageTable(num_pages=9, max_seqs=3, max_pages_per_seq=4)
    a, b = pt.alloc(), pt.alloc()
    pt.commit(pt.reserve([a, b], 20)[0], 20)
    owned = lambda: [pt.table[s][:pt.pages_of[s]] for s in range(3)]
    before = (pt.pages_free, owned(), pt.lengths[:])
    slots, _, taken = pt.reserve([b, a], 30)
    assert taken == [2, 2] and pt.pages_free == 1
    got = owned()
    pt.rollback(slots, taken)
    assert (pt.pages_free, owned(), pt.lengths[:]) == before
    slots, _, taken = pt.reserve([b, a], 30)
    assert owned() == got


def test_max_len_bounds_the_mirrored_lengths():
    """What every call hands the library as max_len is the room of a table row - a bound on every length the allocator can reach,
    and on lens[b] + n of every append it lets through."""
    pt = PageTable(num_pages=64, max_seqs=2, max_pages_per_seq=5)
    assert pt.max_len == 80 == PAGE_KEYS * 5 and (pt.max_len + 15) // 16 <= len(pt.table[0])
    a, b = pt.alloc(), pt.alloc()
    for seqs, n in [([a], 37), ([a, b], 1), ([b], 60), ([a], 42)]:
        slots, before, _ = pt.reserve(seqs, n)
        assert all(x + n <= pt.max_len for x in before)
        pt.commit(slots, n)
    assert pt.length(a) == 80 and pt.length(b) == 61 and max(pt.lengths) <= pt.max_len
    with pytest.raises(RuntimeError):
        pt.reserve([a], 1)  # the 81st key
    with pytest.raises(RuntimeError):
        pt.reserve([b], 20)


def test_public_names_and_covers():
    import json

    import torch

    import lqer_amd
    from lqer_amd import PagedKVCache, QuantizedKVCache

    assert lqer_amd.PagedKVCache is PagedKVCache and callable(lqer_amd.attention_flexible_paged)  # (importable from the package)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    for d, dt in [(16, torch.float16), (128, torch.bfloat16), (24, torch.float16), (160, torch.float32), (64, torch.float64)]:
        assert PagedKVCache.covers(cfg, cfg, d, dt) == QuantizedKVCache.covers(cfg, cfg, d, dt)
    with pytest.raises(NotImplementedError):  # (raised before any allocation: no device is needed)
        PagedKVCache(8, 2, 2, 24, cfg, cfg, torch.float16, "cuda:0")

"""Sliding-window attention over the paged KV pool (lqer_attention_q_decode_paged_window: csrc/attn_decode.hip with the window rule;
lqer_amd.kvcache.PageTable.release, PagedKVCache(window=...)), the part that needs no GPU: the export is declared, exported and bound
with the ABI version unchanged, every refusal comes with its code and a message before anything touches a device, and the allocator
keeps its books when sequences forget their oldest pages - alone, over shared pages, through forks, frees and refused appends."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from lqer_amd import _lib
from lqer_amd.kvcache import PAGE_KEYS, PagedKVCache, PageTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
NAME = "lqer_attention_q_decode_paged_window"


def test_export_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    assert NAME in _lib.SIGNATURES
    assert re.search(r"\bint %s\s*\(" % NAME, hdr)
    getattr(_lib.lib(), NAME)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # an additive export
    # lqer_attention_q_decode_paged's argument list plus the window
    res, args = _lib.SIGNATURES["lqer_attention_q_decode_paged"]
    assert _lib.SIGNATURES[NAME] == (res, args + [C.c_int64])
    decl = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, hdr).group(1)
    base = re.search(r"\bint lqer_attention_q_decode_paged\s*\(([^;]*)\);", hdr).group(1)
    norm = lambda s: " ".join(s.split())
    assert norm(decl) == norm(base) + ", int64_t window"


def _fmt(block=16, width=8):
    return _lib.QFmt(_lib.Q_MXINT, width, block, 8, 127)


def _attend(window, causal=1, q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000,
            lens=0x400000, max_len=64, out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=2, heads=4, kv=4, S=1, D=64, fmts=None):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = (C.c_int64 * 3)(heads * S * D, S * D, D)
    rc = getattr(L, NAME)(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, _lib.F16, batch, heads, kv, S, D, st, st,
                          0.125, causal, *[C.byref(f) for f in fmts], ws, ws_bytes, None, window)
    return rc, L.lqer_last_error().decode()


WS_OK = _lib.lib().lqer_attention_q_decode_paged_workspace_bytes(2, 4, 4, 1, 64, 64)


@pytest.mark.parametrize("case, kwargs, want, word", [
    # the window's own
    ("window = 0", dict(window=0), E_INVALID, "window"),
    ("negative window", dict(window=-5), E_INVALID, "window"),
    ("window without causal", dict(window=8, causal=0), E_INVALID, "causal"),
    ("window = 0 in a call with nothing to do", dict(window=0, batch=0), E_INVALID, "window"),
    ("window before the formats", dict(window=0, fmts=[_fmt(), _fmt(32), _fmt(), _fmt()]), E_INVALID, "window"),
    # lqer_attention_q_decode_paged's, which still apply (the pointers are made up: a call that got past them would fault)
    ("S = 9", dict(window=8, S=9), E_UNSUPPORTED, "query rows"),
    ("D = 24", dict(window=8, D=24), E_UNSUPPORTED, "head dim"),
    ("P block 32", dict(window=8, fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED, "quantizer"),
    ("null q", dict(window=8, q=None), E_INVALID, "null"),
    ("null workspace", dict(window=8, ws=None), E_INVALID, "null"),
    ("short workspace", dict(window=8, ws_bytes=WS_OK - 1), E_INVALID, "workspace"),
    ("workspace not 16-byte aligned", dict(window=8, ws=0x50008), E_INVALID, "aligned"),
    ("null block_table", dict(window=8, tbl=None), E_INVALID, "KV pool"),
    ("null lens", dict(window=8, lens=None), E_INVALID, "KV pool"),
    ("max_len > 16 table_stride", dict(window=8, max_len=65), E_INVALID, "KV pool"),
    ("short pool", dict(window=8, pool_bytes=1000), E_INVALID, "KV pool"),
    ("max_len > 2^30", dict(window=1 << 40, max_len=(1 << 30) + 1, stride=1 << 27, ws_bytes=1 << 62), E_UNSUPPORTED, "2^30"),
])
def test_refusals_before_any_gpu_call(case, kwargs, want, word):
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention_q_decode_paged_window" in msg and word in msg and len(msg) > 20, (case, msg)


def test_a_short_workspace_names_the_size_function_that_exists():
    rc, msg = _attend(window=8, ws_bytes=WS_OK - 1)
    assert rc == E_INVALID and "(lqer_attention_q_decode_paged_workspace_bytes)" in msg and f"< {WS_OK} B" in msg, msg


def test_nothing_to_do_is_ok_with_a_valid_window():
    """batch = 0 returns before any pointer is looked at - the unwindowed call's rule."""
    assert _attend(window=8, batch=0, q=None, out=None, ws=None)[0] == 0
    assert _attend(window=1 << 62, batch=0)[0] == 0


# ---- the allocator -----------------------------------------------------------------------------------------------------------------
def _books(pt):
    return (pt.pages_free, pt.pages_shared, [row[:] for row in pt.table], pt.pages_of[:], pt.released[:], pt.lengths[:], pt._free_pages[:],
            pt._free_slots[:], dict(pt._slot), pt._next_seq, pt._owners.tolist())


def _live_books(pt):
    """_books with every row cut at its entries in use: a rolled-back reservation leaves what it wrote beyond them, and nothing reads it."""
    bk = _books(pt)
    return bk[:2] + ([row[:n] for row, n in zip(bk[2], bk[3])],) + bk[3:]


def _grown(pt, n):
    seq = pt.alloc()
    pt.commit(pt.reserve([seq], n)[0], n)
    return seq


def _held(pt, seq):
    s = pt.slot(seq)
    return pt.table[s][pt.released[s]:pt.pages_of[s]]


def _consistent(pt):
    """Every page is free or owned, never both, and a page's count is the number of live rows that hold it."""
    held = [p for seq in pt._slot for p in _held(pt, seq)]
    counts = [held.count(p) for p in range(pt.num_pages)]
    assert counts == pt._owners.tolist()
    assert sorted(pt._free_pages) == [p for p in range(pt.num_pages) if counts[p] == 0]


def test_release_returns_exactly_the_pages_wholly_below_the_key():
    pt = PageTable(num_pages=10, max_seqs=2, max_pages_per_seq=6)
    a = _grown(pt, 70)  # pages 0 .. 3 full, 4 open
    assert _held(pt, a) == [0, 1, 2, 3, 4] and pt.pages_free == 5
    for key in (0, 1, 15, -40):
        assert pt.release(a, key) == [] and pt.released[pt.slot(a)] == 0
    assert pt.release(a, 33) == [0, 1]  # keys 32 is on page 2: it stays
    assert pt.pages_free == 7 and pt._free_pages[-2:] == [0, 1] and pt.pages_held(a) == 3 and _held(pt, a) == [2, 3, 4]
    assert pt.table[pt.slot(a)][:5] == [0, 1, 2, 3, 4] and pt.pages_of[pt.slot(a)] == 5 and pt.length(a) == 70  # the row keeps its entries
    assert pt.release(a, 47) == [] and pt.release(a, 10) == [] and pt.released[pt.slot(a)] == 2  # nothing more, and never backwards
    assert pt.release(a, 48) == [2]
    assert pt.release(a, 1000) == [3]  # full pages only: the open block at 70 // 16 stays whatever the key
    assert _held(pt, a) == [4] and pt.pages_free == 9
    _consistent(pt)
    with pytest.raises(KeyError):
        pt.release(7, 16)
    # the freed pages serve the sequence's own growth; the stale entries stay in the row
    pt.commit(pt.reserve([a], 20)[0], 20)
    assert pt.table[pt.slot(a)] == [0, 1, 2, 3, 4, 3] and _held(pt, a) == [4, 3]
    _consistent(pt)
    pt.free(a)
    assert pt.pages_free == 10 and pt._owners.tolist() == [0] * 10 and pt.released == [0, 0]
    _consistent(pt)


def test_unrelease_puts_the_books_back():
    pt = PageTable(num_pages=8, max_seqs=3, max_pages_per_seq=6)
    a = _grown(pt, 70)
    (b,), _, _, _ = pt.fork([a])
    pt.release(b, 16)  # page 0 is a's alone from here
    before = _books(pt)
    first = pt.released[pt.slot(a)]
    freed = pt.release(a, 50)  # page 0 goes back, pages 1 and 2 stay with b
    assert freed == [0] and pt.released[pt.slot(a)] == 3
    pt.unrelease(a, first, freed)
    assert _books(pt) == before
    _consistent(pt)


def test_shared_pages_go_back_only_with_the_last_owner():
    pt = PageTable(num_pages=10, max_seqs=3, max_pages_per_seq=6)
    a = _grown(pt, 70)
    (b,), _, _, _ = pt.fork([a])  # shares pages 0 .. 3, page 5 for its open block
    assert pt.pages_shared == 4 and pt.pages_free == 4
    assert pt.release(a, 32) == [] and pt.pages_free == 4 and pt.pages_shared == 2 and pt._owners[:4].tolist() == [1, 1, 2, 2]
    _consistent(pt)
    assert pt.release(b, 48) == [0, 1] and pt.pages_free == 6 and pt._owners[:4].tolist() == [0, 0, 1, 2]
    assert pt.release(a, 48) == [2] and pt.pages_shared == 1
    _consistent(pt)


def _trimmed_parent_and_child():
    """a: 70 keys, its first two pages released and taken by c; b: a fork of the trimmed a."""
    pt = PageTable(num_pages=10, max_seqs=5, max_pages_per_seq=6)
    a = _grown(pt, 70)
    assert pt.release(a, 32) == [0, 1]
    c = _grown(pt, 20)
    assert sorted(_held(pt, c)) == [0, 1]  # the pages a's stale entries still name
    (b,), _, _, _ = pt.fork([a])
    return pt, a, b, c


def test_forking_a_trimmed_parent_counts_live_entries_only():
    pt, a, b, c = _trimmed_parent_and_child()
    assert pt._owners[:5].tolist() == [1, 1, 2, 2, 1]  # pages 0, 1: c's alone - not raised by the fork
    sa, sb = pt.slot(a), pt.slot(b)
    assert pt.released[sb] == pt.released[sa] == 2 and pt.pages_of[sb] == 5 and pt.length(b) == 70
    assert pt.table[sb][:4] == pt.table[sa][:4] and pt.table[sb][4] != pt.table[sa][4]
    assert pt.pages_held(b) == 3 and pt.pages_shared == 2
    _consistent(pt)
    # the child goes on releasing on its own
    assert pt.release(b, 64) == [] and pt.release(a, 64) == [2, 3]
    _consistent(pt)


@pytest.mark.parametrize("order", ["parent first", "child first"])
def test_free_of_parent_and_child_in_either_order(order):
    pt, a, b, c = _trimmed_parent_and_child()
    for seq in ((a, b) if order == "parent first" else (b, a)):
        pt.free(seq)
        _consistent(pt)
        assert sorted(_held(pt, c)) == [0, 1] and pt._owners[:2].tolist() == [1, 1]  # the stale entries took nothing from c
    pt.free(c)
    assert pt.pages_free == 10 and sorted(pt._free_pages) == list(range(10)) and pt._owners.tolist() == [0] * 10
    assert sorted(pt._free_slots) == list(range(5)) and pt.released == [0] * 5


def test_rollback_fork_and_snapshot_honour_the_released_count():
    pt, a, b, c = _trimmed_parent_and_child()
    before = _books(pt)
    children, _, _, _ = pt.fork([a, b])
    assert pt.released[pt.slot(children[0])] == 2 and pt._owners[:4].tolist() == [1, 1, 4, 4] and pt.pages_free == 2
    pt.rollback_fork(children)
    after = _books(pt)
    live = [pt.slot(s) for s in (a, b, c)]
    strip = lambda bk: bk[:2] + ([bk[2][s] for s in live],) + bk[3:]  # (rows of free slots keep what was written there)
    assert strip(after) == strip(before)
    snap = pt.snapshot([b])
    pt.release(a, 64), pt.free(b)
    assert _books(pt) != before
    pt.restore(snap)
    assert strip(_books(pt)) == strip(before)
    _consistent(pt)


# ---- PagedKVCache(window=W).append: the release rule, its undo and the bound - on the host, the launch replaced ------------------------
def _host_cache(num_pages, max_seqs, window, max_pages_per_seq, launch=None):
    """A PagedKVCache whose buffers live in host memory and whose launch is `launch` (default: nothing): append()'s own bookkeeping runs
    as it is, and no device is needed or touched."""
    with open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")) as fh:
        cfg = json.load(fh)
    cache = PagedKVCache(num_pages, max_seqs, 2, 16, cfg, cfg, torch.float16, "cpu", max_pages_per_seq=max_pages_per_seq, window=window)
    cache._launch_append = launch or (lambda *a: None)
    return cache


def _kv(batch, n):
    return torch.zeros(batch, 2, n, 16, dtype=torch.float16)


@pytest.mark.parametrize("W", [1, 16, 33])
def test_a_sequence_holds_at_most_W_plus_37_over_16_pages(W):
    """300 one-key appends to two sequences in a pool of exactly 2 ((W + 37) // 16) pages: never out of pages, the bound is reached,
    and what is released is exactly what no call of up to 8 query rows can see."""
    bound = (W + 37) // 16
    cache = _host_cache(2 * bound, 2, W, max_pages_per_seq=19)
    seqs = [cache.alloc(), cache.alloc()]
    most = 0
    for t in range(1, 301):
        cache.append(seqs, _kv(2, 1), _kv(2, 1))
        for s in seqs:
            assert cache.length(s) == t and cache.pages_held(s) <= bound
            assert cache.pt.released[cache.pt.slot(s)] == max(0, (t - W - 7) // 16)
            assert 16 * cache.pt.released[cache.pt.slot(s)] <= max(0, t - 8 - W + 1)  # the first key of a call of 8 rows
        most = max(most, cache.pages_held(seqs[0]))
        _consistent(cache.pt)
    assert most == bound
    for s in seqs:
        cache.free(s)
    assert cache.pages_free == 2 * bound


def test_an_append_never_releases_the_blocks_it_rewrites():
    """A long append to a short window: T_after - W - 7 lies beyond the open block, the bound is 16 (T_before // 16)."""
    cache = _host_cache(12, 1, 4, max_pages_per_seq=12)
    s = cache.alloc()
    cache.append([s], _kv(1, 21), _kv(1, 21))
    assert cache.pt.released[0] == 0
    cache.append([s], _kv(1, 100), _kv(1, 100))  # 21 -> 121: pages below 16 (21 // 16) = 16 only
    assert cache.pt.released[0] == 1 and cache.pages_held(s) == 7
    cache.append([s], _kv(1, 1), _kv(1, 1))      # 122 - 4 - 7 = 111 -> six pages
    assert cache.pt.released[0] == 6 and cache.pages_held(s) == 2


def test_a_refused_append_leaves_the_books_as_they_were():
    def refuse(*a):
        raise RuntimeError("the launch is refused")

    for what, launch, exc in (("the reservation", None, RuntimeError), ("the launch", refuse, RuntimeError)):
        cache = _host_cache(6, 3, 8, max_pages_per_seq=8)
        a, b, c = cache.alloc(), cache.alloc(), cache.alloc()
        cache.append([a, b], _kv(2, 40), _kv(2, 40))  # 3 + 3 pages: none free
        before = _live_books(cache.pt)
        cache._launch_append = launch or cache._launch_append
        # a and b each release two pages (40 + 9 - 8 - 7 = 34 -> keys below 32) and need one; c needs one
        with pytest.raises(exc):
            cache.append([a, b, c], _kv(3, 9 if launch else 90), _kv(3, 9 if launch else 90))  # (90 keys: beyond max_pages_per_seq)
        assert _live_books(cache.pt) == before, what
        for seqs, k in (([a, a], _kv(2, 9)), ([a, 7], _kv(2, 9))):  # named twice; unknown: refused before anything is released
            with pytest.raises((ValueError, KeyError)):
                cache.append(seqs, k, k)
            assert _live_books(cache.pt) == before, what
    # ... and the same call goes through once it can
    cache = _host_cache(6, 3, 8, max_pages_per_seq=8)
    a, b, c = cache.alloc(), cache.alloc(), cache.alloc()
    cache.append([a, b], _kv(2, 40), _kv(2, 40))
    cache.append([a, b, c], _kv(3, 9), _kv(3, 9))  # the pages a and b let go serve all three
    assert [cache.pages_held(s) for s in (a, b, c)] == [2, 2, 1] and cache.pages_free == 1
    _consistent(cache.pt)


def test_python_refusals_on_the_host():
    cache = _host_cache(8, 2, 8, max_pages_per_seq=8)
    s = cache.alloc()
    cache.append([s], _kv(1, 40), _kv(1, 40))
    cache.append([s], _kv(1, 1), _kv(1, 1))
    assert cache.pt.released[0] == 1
    with pytest.raises(ValueError, match="released"):
        cache.to_dense(s)
    with pytest.raises(ValueError, match="released"):
        cache.dequantized(s)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            _host_cache(4, 1, bad, max_pages_per_seq=4)
    assert _host_cache(4, 1, None, max_pages_per_seq=4).window is None

"""Forking sequences over shared pages of the paged KV pool (lqer_kv_pool_fork: csrc/kv_cache.hip; lqer_amd.kvcache.PageTable.fork), the
part that needs no GPU: the export is declared, exported and bound, every refusal comes with its code and a message before anything
touches the device, the allocator's owner counts keep a shared page live until its last owner goes - all or nothing, with a rollback -
and a run without any fork leaves the books the allocator left before it counted owners."""
import ctypes as C
import os
import re

import pytest

from lqer_amd import _lib
from lqer_amd.kvcache import PAGE_KEYS, PageTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
up = lambda v: (v + 255) // 256 * 256
POOL_OK = 2 * up(8 * 4 * 16 * 64) + 2 * up(8 * 4 * 64) + up(4 * 4 * 16 * 64 * 2)  # pages 8, slots 4, kv 4, D 64, fp16 (include/lqer_hip.h)


def test_export_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    assert "lqer_kv_pool_fork" in _lib.SIGNATURES
    assert re.search(r"\bint lqer_kv_pool_fork\s*\(", hdr)
    getattr(_lib.lib(), "lqer_kv_pool_fork")
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # an additive export
    vp, sz, i, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64
    # lqer_kv_pool_gather's description of the pool, then the three device arrays, the number of pairs and the stream
    assert _lib.SIGNATURES["lqer_kv_pool_fork"] == (i, _lib.SIGNATURES["lqer_kv_pool_gather"][1][:9] + [vp, vp, vp, i64, vp])
    assert _lib.SIGNATURES["lqer_kv_pool_fork"][1][:9] == [vp, sz, i, i64, i64, i64, i64, vp, i64]
    assert _lib.lib().lqer_kv_pool_bytes(_lib.F16, 8, 4, 4, 64) == POOL_OK
    assert "no page belongs to\n * two live sequences" not in hdr and "belongs to it alone" in hdr  # the invariant that allows sharing


def _fork(pool=0x100000, pool_bytes=1 << 24, dtype=_lib.F16, pages=8, slots=4, kv=4, D=64, tbl=0x200000, stride=4, src=0x300000, dst=0x400000,
          lens=0x500000, n=2):
    L = _lib.lib()
    rc = L.lqer_kv_pool_fork(pool, pool_bytes, dtype, pages, slots, kv, D, tbl, stride, src, dst, lens, n, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("null pool", dict(pool=None), E_INVALID),
    ("null block_table", dict(tbl=None), E_INVALID),
    ("null src_slots", dict(src=None), E_INVALID),
    ("null dst_slots", dict(dst=None), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("n = 0", dict(n=0), E_INVALID),
    ("negative n", dict(n=-3), E_INVALID),
    ("pages = 0", dict(pages=0), E_INVALID),
    ("slots = 0", dict(slots=0), E_INVALID),
    ("kv_heads = 0", dict(kv=0), E_INVALID),
    ("table_stride = 0", dict(stride=0), E_INVALID),
    ("D = 0", dict(D=0), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
    ("pool not 16-byte aligned", dict(pool=0x100008), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("n x kv_heads beyond the grid", dict(n=1 << 29), E_UNSUPPORTED),
    ("n x kv_heads would overflow", dict(n=1 << 62), E_UNSUPPORTED),
])
def test_fork_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _fork(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "kv_pool_fork" in msg and "KV pool" in msg and len(msg) > 20, (case, msg)
    if "dtype" in kwargs or kwargs.get("D"):  # ... which are what lqer_kv_pool_bytes rejects
        assert _lib.lib().lqer_kv_pool_bytes(kwargs.get("dtype", _lib.F16), 8, 4, 4, kwargs.get("D", 64)) == 0


def test_the_first_grid_that_is_refused():
    """2^31 - 1 workgroups along x, one per (pair, kv head): the smallest n beyond it at 4 kv heads."""
    rc, msg = _fork(n=((1 << 31) - 1) // 4 + 1)
    assert rc == E_UNSUPPORTED and "launch grid" in msg, (rc, msg)


# ---- the allocator ---------------------------------------------------------------------------------------------------------------------
def _books(pt):
    return (pt.pages_free, pt.pages_shared, [row[:] for row in pt.table], pt.pages_of[:], pt.lengths[:], pt._free_pages[:], pt._free_slots[:],
            dict(pt._slot), pt._next_seq, pt._owners.tolist())


def _owned(pt, seq):
    s = pt.slot(seq)
    return pt.table[s][:pt.pages_of[s]]


def _grown(pt, n):
    seq = pt.alloc()
    if n:
        pt.commit(pt.reserve([seq], n)[0], n)
    return seq


@pytest.mark.parametrize("length", [0, 5, 16, 37])
def test_fork_counts(length):
    """Two children of one parent: they share its floor(L / 16) full pages, and each takes one page of its own iff L % 16 != 0."""
    pt = PageTable(num_pages=12, max_seqs=4, max_pages_per_seq=4)
    a = _grown(pt, length)
    full, tail, used = length // PAGE_KEYS, int(length % PAGE_KEYS != 0), (length + 15) // PAGE_KEYS
    assert pt.pages_free == 12 - used and pt.pages_shared == 0
    children, src, dst, lens = pt.fork([a, a])
    assert children == [1, 2] and src == [pt.slot(a)] * 2 and dst == [pt.slot(c) for c in children] and lens == [length] * 2
    assert len({pt.slot(a), *dst}) == 3
    assert pt.pages_free == 12 - used - 2 * tail and pt.pages_shared == full
    for c in children:
        assert pt.length(c) == length and pt.pages_of[pt.slot(c)] == used
        assert _owned(pt, c)[:full] == _owned(pt, a)[:full]  # the full pages: the parent's
    tails = [_owned(pt, s)[full] for s in (a, *children)] if tail else []
    assert len(set(tails)) == len(tails)  # the open block's page: everyone's own
    assert [pt._owners[p] for p in _owned(pt, a)] == [3] * full + [1] * tail
    live = {p for s in (a, *children) for p in _owned(pt, s)}
    assert len(live) == 12 - pt.pages_free == used + 2 * tail  # every page is either free or owned
    # the sequences then grow apart, each on pages of its own
    for s in (a, *children):
        pt.commit(pt.reserve([s], 20)[0], 20)
    assert pt.pages_shared == full
    new = [p for s in (a, *children) for p in _owned(pt, s)[full:]]
    assert len(set(new)) == len(new) and not set(new) & set(_owned(pt, a)[:full])


def test_free_keeps_shared_pages_until_the_last_owner():
    pt = PageTable(num_pages=10, max_seqs=4, max_pages_per_seq=4)
    a = _grown(pt, 37)  # pages 0, 1 full, 2 open
    assert _owned(pt, a) == [0, 1, 2]
    (b,), _, _, _ = pt.fork([a])
    assert _owned(pt, b) == [0, 1, 3] and pt.pages_free == 6 and pt.pages_shared == 2
    (c,), _, _, _ = pt.fork([b])  # a fork of a fork
    assert _owned(pt, c) == [0, 1, 4] and pt.pages_free == 5 and [pt._owners[p] for p in range(5)] == [3, 3, 1, 1, 1]
    pt.free(a)
    assert pt.pages_free == 6 and pt._free_pages[-1] == 2 and pt.pages_shared == 2  # only a's own page came back
    with pytest.raises(KeyError):
        pt.length(a)
    assert _owned(pt, b) == [0, 1, 3] and _owned(pt, c) == [0, 1, 4] and pt.length(b) == pt.length(c) == 37
    pt.free(c)
    assert pt.pages_free == 7 and pt.pages_shared == 0 and [pt._owners[p] for p in range(5)] == [1, 1, 0, 1, 0]
    pt.free(b)  # the last owner: its pages in the order free() has always used, the last page first
    assert pt.pages_free == 10 == pt.num_pages and pt._free_pages[-3:] == [3, 1, 0] and pt._owners.tolist() == [0] * 10
    assert sorted(pt._free_pages) == list(range(10)) and sorted(pt._free_slots) == list(range(4))
    d = _grown(pt, 48)
    assert _owned(pt, d) == [0, 1, 3]


def test_fork_refuses_with_nothing_taken():
    pt = PageTable(num_pages=5, max_seqs=4, max_pages_per_seq=3)
    a, b = _grown(pt, 20), _grown(pt, 33)  # 2 + 3 pages: none left
    before = _books(pt)
    for what, parents, exc in [("out of pages", [a], RuntimeError), ("out of pages: both need one", [a, b], RuntimeError),
                               ("out of slots", [a, a, a], RuntimeError), ("unknown parent", [a, 9], KeyError)]:
        with pytest.raises(exc):
            pt.fork(parents)
        assert _books(pt) == before, what
    pt.free(b)
    with pytest.raises(KeyError):
        pt.fork([b])  # freed
    before = _books(pt)
    with pytest.raises(RuntimeError):
        pt.fork([a, a, a, a])  # three slots, not four - though the pages would do
    assert _books(pt) == before
    kids, _, _, _ = pt.fork([a, a, a])
    assert pt.pages_free == 0 and pt.pages_shared == 1 and len(kids) == 3
    with pytest.raises(RuntimeError):
        pt.alloc()
    # a full parent needs no page: the fork goes through with none free
    pt = PageTable(num_pages=2, max_seqs=3, max_pages_per_seq=2)
    a = _grown(pt, 32)
    kids, _, _, _ = pt.fork([a, a])
    assert pt.pages_free == 0 and pt.pages_shared == 2 and all(_owned(pt, k) == _owned(pt, a) for k in kids)


def test_rollback_of_a_fork_whose_launch_was_refused():
    pt = PageTable(num_pages=9, max_seqs=5, max_pages_per_seq=4)
    a, b = _grown(pt, 37), _grown(pt, 16)
    before = _books(pt)
    children, src, dst, lens = pt.fork([a, b, a])
    got = (children, dst, [_owned(pt, c) for c in children])
    assert pt.pages_free == 3 and pt.pages_shared == 3
    pt.rollback_fork(children)
    after = _books(pt)
    # (rows of free slots keep what was written there, like a rolled-back reserve's: nothing reads them)
    strip = lambda bk: bk[:2] + ([bk[2][s] for s in (pt.slot(a), pt.slot(b))],) + bk[3:]
    assert strip(after) == strip(before)
    again = pt.fork([a, b, a])
    assert (again[0], again[2], [_owned(pt, c) for c in again[0]]) == got  # the same ids, slots and pages
    slots, _, taken = pt.reserve([a], 20)  # ... and the next reservation after a rollback takes the same pages
    mine = _owned(pt, a)
    pt.rollback(slots, taken)
    assert pt.reserve([a], 20)[2] == taken == [1] and _owned(pt, a) == mine


def test_snapshot_and_restore_put_freed_sequences_back():
    """What reorder() leans on: the dropped sequences are freed first so that their pages and slots can serve the forks, and a call
    that cannot be served after all leaves the books as they were."""
    pt = PageTable(num_pages=4, max_seqs=3, max_pages_per_seq=3)
    a = _grown(pt, 21)
    (b,), _, _, _ = pt.fork([a])  # a: [0, 1], b: [0, 2]; one page free
    c = _grown(pt, 5)             # none free
    before = _books(pt)
    snap = pt.snapshot([b, c])
    pt.free(b), pt.free(c)        # b gives back its own page (page 0 stays with a) and c its one: two pages, two slots
    kids, _, _, _ = pt.fork([a, a])
    assert pt.pages_free == 0 and pt.pages_shared == 1 and [pt._owners[p] for p in _owned(pt, a)] == [3, 1]
    pt.restore(snap)
    assert _books(pt) == before and pt.length(b) == 21 and pt.length(c) == 5
    snap = pt.snapshot([c])
    pt.free(c)
    with pytest.raises(RuntimeError):
        pt.fork([a, a])           # c's page and slot serve one fork, not two
    pt.restore(snap)
    assert _books(pt) == before


def test_no_fork_no_change():
    """alloc / reserve / rollback / free with no fork in between: ids, table rows, page counts, lengths and the order of both free
    stacks are those of the allocator before it counted owners (values recorded from a run of that code)."""
    pt = PageTable(num_pages=12, max_seqs=4, max_pages_per_seq=5)
    a, b, c = pt.alloc(), pt.alloc(), pt.alloc()
    pt.commit(pt.reserve([a, b], 20)[0], 20)
    pt.commit(pt.reserve([c, a], 13)[0], 13)
    slots, _, taken = pt.reserve([b], 30)
    pt.rollback(slots, taken)
    pt.free(a)
    d = pt.alloc()
    pt.commit(pt.reserve([d, b], 37)[0], 37)
    pt.free(c)
    pt.commit(pt.reserve([d], 1)[0], 1)
    pt.free(b)
    e = pt.alloc()
    pt.commit(pt.reserve([e], 16)[0], 16)
    assert (a, b, c, d, e) == (0, 1, 2, 3, 4)
    assert pt.table == [[0, 1, 5, 0, 0], [2, 3, 6, 7, 0], [4, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert pt.pages_of == [3, 1, 0, 0] and pt.lengths == [38, 16, 0, 0]
    assert pt._free_pages == [11, 10, 9, 8, 4, 7, 6, 3] and pt._free_slots == [3, 2]
    assert pt.pages_shared == 0 and int(pt._owners.sum()) == 4 == 12 - pt.pages_free

"""Copying pages between paged KV pools and swapping sequences out and in (lqer_kv_pool_copy: csrc/kv_cache.hip; lqer_amd.kvcache.PageTable
.export / .adopt / .rollback_adopt), the part that needs no GPU: the export is declared, exported and bound, every refusal comes with its
code and a message before anything touches the device, and the host books carry shared pages, owner counts and released pages from one
table to another - all or nothing, with a rollback - while a run without export or adopt leaves the books as they were."""
import ctypes as C
import os
import re

import pytest

from lqer_amd import _lib
from lqer_amd.kvcache import PAGE_KEYS, PageTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SRC, DST = 0x1000000, 0x8000000  # made-up, 16-byte aligned, far apart
ROOM = ((1 << 31) - 1) // 4      # page and slot pairs one launch grid takes at 4 kv heads


def fmt(kind=_lib.Q_MXINT, width=4, block=16, exp_width=8, exp_bias=127):
    return _lib.QFmt(kind, width, block, exp_width, exp_bias)


def need(pages, slots, kv=4, D=64, dtype=_lib.F16, fmts=None):
    L = _lib.lib()
    if fmts is None:
        return L.lqer_kv_pool_bytes(dtype, pages, slots, kv, D)
    return L.lqer_kv_pool_bytes_fmt(dtype, pages, slots, kv, D, C.byref(fmts[0]), C.byref(fmts[1]))


def test_export_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    assert "lqer_kv_pool_copy" in _lib.SIGNATURES
    m = re.search(r"\bint lqer_kv_pool_copy\s*\(([^;]*)\);", hdr)
    assert m, "lqer_kv_pool_copy is not declared in include/lqer_hip.h"
    getattr(_lib.lib(), "lqer_kv_pool_copy")
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # an additive export
    names = [a.split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
    assert names == ["src_pool", "src_bytes", "src_pages", "src_slots", "dst_pool", "dst_bytes", "dst_pages", "dst_slots", "dtype", "kv_heads", "D",
                     "src_page_ids", "dst_page_ids", "n_pages", "src_slot_ids", "dst_slot_ids", "n_slots", "k_fmt", "v_fmt", "stream"]
    vp, sz, i, i64, qp = C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.POINTER(_lib.QFmt)
    side = [vp, sz, i64, i64]
    assert _lib.SIGNATURES["lqer_kv_pool_copy"] == (i, side + side + [i, i64, i64] + [vp, vp, i64] * 2 + [qp, qp, vp])
    for word in ("dst_page_ids are distinct", "disjoint", "no destination page or slot is also a source"):  # the caller's contract
        assert word in hdr, word


def _copy(src=SRC, src_bytes=1 << 24, src_pages=8, src_slots=4, dst=DST, dst_bytes=1 << 24, dst_pages=6, dst_slots=3, dtype=_lib.F16, kv=4, D=64,
          sp=0x300000, dp=0x400000, n_pages=2, ss=0x500000, ds=0x600000, n_slots=1, k_fmt=None, v_fmt=None):
    L = _lib.lib()
    byref = lambda f: None if f is None else C.byref(f)
    rc = L.lqer_kv_pool_copy(src, src_bytes, src_pages, src_slots, dst, dst_bytes, dst_pages, dst_slots, dtype, kv, D, sp, dp, n_pages, ss, ds,
                             n_slots, byref(k_fmt), byref(v_fmt), None)
    return rc, L.lqer_last_error().decode()


C4 = _lib.Q_MXINT_C4
REFUSALS = [
    ("null source pool", dict(src=None), E_INVALID),
    ("null destination pool", dict(dst=None), E_INVALID),
    ("source not 16-byte aligned", dict(src=SRC + 8), E_INVALID),
    ("destination not 16-byte aligned", dict(dst=DST + 4), E_INVALID),
    ("short source", dict(src_bytes=need(8, 4) - 1), E_INVALID),
    ("short destination", dict(dst_bytes=need(6, 3) - 1), E_INVALID),
    ("destination long enough for bytes, short for nibbles' sibling", dict(dst_bytes=need(6, 3, fmts=(fmt(C4), fmt(C4)))), E_INVALID),
    ("short nibble destination", dict(dst_bytes=need(6, 3, fmts=(fmt(C4), fmt(C4))) - 1, k_fmt=fmt(C4), v_fmt=fmt(C4)), E_INVALID),
    ("negative n_pages", dict(n_pages=-1), E_INVALID),
    ("negative n_slots", dict(n_slots=-2), E_INVALID),
    ("null src_page_ids", dict(sp=None), E_INVALID),
    ("null dst_page_ids", dict(dp=None), E_INVALID),
    ("null src_slot_ids", dict(ss=None), E_INVALID),
    ("null dst_slot_ids", dict(ds=None), E_INVALID),
    ("null page ids, no slots", dict(sp=None, dp=None, n_slots=0), E_INVALID),
    ("k_fmt alone", dict(k_fmt=fmt()), E_INVALID),
    ("v_fmt alone", dict(v_fmt=fmt(C4)), E_INVALID),
    ("destination inside the source", dict(dst=SRC + 256), E_INVALID),
    ("source inside the destination", dict(src=DST + need(6, 3) - 16), E_INVALID),
    ("one buffer, other page count", dict(dst=SRC, dst_pages=8, dst_slots=3), E_INVALID),
    ("one buffer, other slot count", dict(dst=SRC, dst_pages=6, dst_slots=4), E_INVALID),
    ("pages = 0", dict(src_pages=0), E_INVALID),
    ("slots = 0", dict(dst_slots=0), E_INVALID),
    ("kv_heads = 0", dict(kv=0), E_INVALID),
    ("D = 0", dict(D=0), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("nibble kind of width 8", dict(k_fmt=fmt(C4, width=8), v_fmt=fmt()), E_UNSUPPORTED),
    ("width 9", dict(k_fmt=fmt(), v_fmt=fmt(width=9)), E_UNSUPPORTED),
    ("block 32", dict(k_fmt=fmt(block=32), v_fmt=fmt()), E_UNSUPPORTED),
    ("another kind", dict(k_fmt=fmt(), v_fmt=fmt(kind=_lib.Q_INT)), E_UNSUPPORTED),
    ("the first grid that is refused: pages", dict(n_pages=ROOM + 1, n_slots=0), E_UNSUPPORTED),
    ("the first grid that is refused: slots", dict(n_pages=0, n_slots=ROOM + 1), E_UNSUPPORTED),
    ("the first grid that is refused: the sum", dict(n_pages=ROOM, n_slots=1), E_UNSUPPORTED),
    ("counts whose sum would overflow", dict(n_pages=1 << 62, n_slots=1 << 62), E_UNSUPPORTED),
]


@pytest.mark.parametrize("case, kwargs, want", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_copy_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _copy(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "kv_pool_copy" in msg and "KV pool" in msg and len(msg) > 20, (case, msg)
    if want == E_UNSUPPORTED and "grid" not in case and "overflow" not in case:  # ... which are what the size functions answer 0 for
        k, v = kwargs.get("k_fmt"), kwargs.get("v_fmt")
        assert need(8, 4, D=kwargs.get("D", 64), dtype=kwargs.get("dtype", _lib.F16), fmts=(k, v) if k is not None else None) == 0
    if "grid" in case:
        assert "launch grid" in msg


@pytest.mark.parametrize("kwargs", [dict(), dict(sp=None, dp=None, ss=None, ds=None), dict(k_fmt=fmt(C4), v_fmt=fmt(C4, width=3)),
                                    dict(k_fmt=fmt(width=8), v_fmt=fmt(C4)), dict(dst=SRC, dst_pages=8, dst_slots=4),
                                    dict(dst=SRC + need(8, 4)), dict(src_bytes=need(8, 4), dst_bytes=need(6, 3))],
                         ids=["plain", "null id arrays", "nibbles", "K bytes V nibbles", "one pool", "back to back", "exact sizes"])
def test_both_counts_zero_validate_and_launch_nothing(kwargs):
    rc, msg = _copy(n_pages=0, n_slots=0, **kwargs)
    assert rc == 0, (rc, msg)


# ---- the books ---------------------------------------------------------------------------------------------------------------------------
def _books(pt):
    return (pt.pages_free, pt.pages_shared, [row[:] for row in pt.table], pt.pages_of[:], pt.lengths[:], pt.released[:], pt._free_pages[:],
            pt._free_slots[:], dict(pt._slot), pt._next_seq, pt._owners.tolist())


def _snap_equal(a, b):
    return all((x == y).all() if hasattr(x, "all") else x == y for x, y in zip(a, b)) and len(a) == len(b)


def _held(pt, seq):
    s = pt.slot(seq)
    return pt.table[s][pt.released[s]:pt.pages_of[s]]


def _grown(pt, n):
    seq = pt.alloc()
    if n:
        pt.commit(pt.reserve([seq], n)[0], n)
    return seq


def _forked():
    """A parent of 40 keys (pages 0, 1 full, 2 open) forked twice, the children grown by 3 and by 30 keys; a loner of 5 keys."""
    pt = PageTable(num_pages=12, max_seqs=5, max_pages_per_seq=6)
    a = _grown(pt, 40)
    (b, c), _, _, _ = pt.fork([a, a])
    pt.commit(pt.reserve([b], 3)[0], 3)
    pt.commit(pt.reserve([c], 30)[0], 30)
    d = _grown(pt, 5)
    return pt, (a, b, c, d)


def test_export_lists_a_shared_page_once_and_changes_nothing():
    pt, (a, b, c, d) = _forked()
    before = _books(pt)
    books = pt.export([b, d, c])
    assert _books(pt) == before
    rows = [_held(pt, s) for s in (b, d, c)]
    assert rows[0][:2] == rows[2][:2] and pt.pages_shared == 2  # the parent's two full pages
    assert books["pages"] == list(dict.fromkeys(rows[0] + rows[1] + rows[2]))  # distinct, in order of first appearance
    assert len(books["pages"]) == 3 + 1 + 3 and len(set(books["pages"])) == 7
    assert [(n, gone) for n, gone, _ in books["seqs"]] == [(43, 0), (5, 0), (70, 0)]
    assert [r for _, _, r in books["seqs"]] == [[0, 1, 2], [3], [0, 1, 4, 5, 6]]
    assert [[books["pages"][i] for i in r] for _, _, r in books["seqs"]] == rows
    for bad, exc in (([a, a], ValueError), ([a, 17], KeyError)):
        with pytest.raises(exc):
            pt.export(bad)
    pt.free(d)
    with pytest.raises(KeyError):
        pt.export([d])
    assert pt.export([_grown(pt, 0)]) == {"pages": [], "seqs": [(0, 0, [])]}


def test_adopt_keeps_shared_pages_owner_counts_and_released():
    pt, (a, b, c, d) = _forked()
    pt.release(c, 40)  # c forgets its first two pages: a and b still hold them
    assert pt.released[pt.slot(c)] == 2 and pt.pages_shared == 2
    books = pt.export([a, b, c, d])
    assert [gone for _, gone, _ in books["seqs"]] == [0, 0, 2, 0] and books["seqs"][2][2][:2] == [0, 0]
    # into another table, whose free stack no longer counts down
    to = PageTable(num_pages=20, max_seqs=6, max_pages_per_seq=7)
    junk = [_grown(to, n) for n in (33, 17, 50)]
    to.free(junk[0]), to.free(junk[1])
    seqs, slots, pages = to.adopt(books)
    assert len(seqs) == 4 and slots == [to.slot(s) for s in seqs] and len(set(pages)) == len(pages) == len(books["pages"])
    assert pages != sorted(pages) and pages != books["pages"]  # no page id survives by construction
    assert [to.length(s) for s in seqs] == [40, 43, 70, 5] and [to.released[x] for x in slots] == [0, 0, 2, 0]
    assert [to.pages_held(s) for s in seqs] == [pt.pages_held(s) for s in (a, b, c, d)]
    assert to.pages_shared == pt.pages_shared == 2
    for new, old in zip(seqs, (a, b, c, d)):  # the same sharing pattern, page for page
        assert [pages.index(p) for p in _held(to, new)] == [books["pages"].index(p) for p in _held(pt, old)]
        assert [int(to._owners[p]) for p in _held(to, new)] == [int(pt._owners[p]) for p in _held(pt, old)]
    assert to.table[slots[2]][:2] == [0, 0]  # released entries: 0, a valid index that nothing reads
    assert to.pages_free == 20 - 4 - len(pages) and int(to._owners.sum()) == sum(to.pages_held(s) for s in seqs) + 4
    # from then on sequences like any other: they grow, and free hands a shared page back with its last owner
    to.commit(to.reserve([seqs[1]], 20)[0], 20)
    free = to.pages_free
    to.free(seqs[0])
    assert to.pages_free == free + 1 and to.pages_shared == 0  # a's open page came back; its full pages stay, now b's alone
    to.free(seqs[1])
    assert to.pages_shared == 0
    for s in (seqs[2], seqs[3], junk[2]):
        to.free(s)
    assert to.pages_free == 20 and to._owners.tolist() == [0] * 20 and sorted(to._free_slots) == list(range(6))


@pytest.mark.parametrize("what, kw", [("out of slots", dict(num_pages=20, max_seqs=3, max_pages_per_seq=6)),
                                      ("out of pages", dict(num_pages=7, max_seqs=5, max_pages_per_seq=6)),
                                      ("beyond max_pages_per_seq", dict(num_pages=20, max_seqs=5, max_pages_per_seq=4))])
def test_adopt_refuses_with_nothing_taken(what, kw):
    pt, seqs = _forked()
    books = pt.export(seqs)  # 4 sequences, 8 distinct pages, the longest row 5 entries
    assert len(books["pages"]) == 8 and max(len(r) for _, _, r in books["seqs"]) == 5
    to = PageTable(**kw)
    x = _grown(to, 3)
    before, snap = _books(to), to.snapshot([x])
    with pytest.raises(RuntimeError, match="adopt"):
        to.adopt(books)
    assert _books(to) == before and _snap_equal(to.snapshot([x]), snap), what
    to.free(x)
    fits = PageTable(num_pages=8, max_seqs=4, max_pages_per_seq=5)  # exactly enough of each
    assert fits.adopt(books)[2] == list(range(8)) and fits.pages_free == 0
    for bad in ({"pages": [0, 1], "seqs": [(16, 0, [0])]}, {"pages": [0], "seqs": [(20, 0, [0, 1])]}, {"pages": [0], "seqs": [(16, 2, [0])]}):
        before = _books(to)
        with pytest.raises(ValueError):
            to.adopt(bad)  # books that name pages they do not list, or list pages nothing names
        assert _books(to) == before


def test_rollback_of_an_adopt_whose_launch_was_refused():
    pt, seqs = _forked()
    pt.release(seqs[2], 40)
    books = pt.export(seqs)
    to = PageTable(num_pages=16, max_seqs=6, max_pages_per_seq=6)
    keep = [_grown(to, n) for n in (20, 40, 9)]
    to.free(keep[1])  # pages 2, 3, 4 back on the stack, out of order
    before = _books(to)
    got = to.adopt(books)
    assert to.pages_free == 16 - 3 - 8 and to.pages_shared == 2
    to.rollback_adopt(got[0])
    after = _books(to)
    live = [to.slot(keep[0]), to.slot(keep[2])]
    # (rows of free slots keep what was written there, like a rolled-back fork's: nothing reads them)
    strip = lambda bk: bk[:2] + ([bk[2][s] for s in live],) + bk[3:]
    assert strip(after) == strip(before)
    assert to.adopt(books) == got  # the same ids, slots and pages
    slots, _, taken = to.reserve([keep[0]], 30)  # ... and the books still serve the others
    assert taken == [2] and to.pages_free == 16 - 3 - 8 - 2


def test_no_export_no_adopt_no_change():
    """alloc / reserve / rollback / fork / release / free with no export or adopt in between: ids, table rows, page counts, lengths and
    the order of both free stacks are those of the allocator before it knew either (values recorded from a run of that code)."""
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
    (f,), _, _, _ = pt.fork([d])
    assert pt.release(d, 32) == [] and pt.release(f, 32) == [0, 1]
    assert pt._free_pages == [11, 10, 9, 8, 4, 7, 6, 0, 1] and pt.table[pt.slot(f)] == [0, 1, 3, 0, 0] and pt.released == [2, 0, 2, 0]
    assert callable(pt.export) and callable(pt.adopt) and callable(pt.rollback_adopt)

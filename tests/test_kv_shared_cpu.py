"""A shared prefix read once per group by the decode attention over the paged KV pool (lqer_attention_q_decode_paged_shared: the GRP
instantiation of csrc/attn_decode.hip's two kernels; lqer_amd.kvcache.PageTable.prefix_groups, attention_flexible_paged(...,
shared_prefix=True)), the part that needs no GPU: the two exports are declared, exported and bound, the chunk length is the kernels'
rule, the groups come out of the host's books as the kernels' contract wants them, the one call builder names the entry with the group
arrays, and every refusal - the library's and Python's - comes before anything touches a device."""
import ctypes as C
import os
import re

import pytest
import torch

from lqer_amd import _lib, attention_flexible_paged, kvcache
from lqer_amd.kvcache import PageTable
from test_kv_paged_call_cpu import _names
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, _fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED, PLAIN = "lqer_attention_q_decode_paged_shared", "lqer_attention_q_decode_paged"
SIG = _lib.SIGNATURES


def chunk_of(t):
    """The rule in plain words (DESIGN, include/lqer_hip.h): 16 ceil(T / 256) clamped to [16, 128]."""
    return 16 * min(max((t + 255) // 256, 1), 8)


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in (SHARED, "lqer_attention_q_decode_chunk"):
        assert name in SIG
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # additive exports
    vp, i64 = C.c_void_p, C.c_int64
    assert SIG[SHARED] == (C.c_int, SIG[PLAIN][1] + [vp, vp, vp, vp, i64])  # the plain call's list plus the four arrays and n_groups
    assert _names(SHARED) == _names(PLAIN) + ["grp_of", "grp_starts", "grp_members", "grp_keys", "n_groups"]
    assert SIG["lqer_attention_q_decode_chunk"] == (C.c_int, [i64, i64])
    assert "lqer_attention_q_decode_paged_shared_workspace_bytes" not in hdr + " ".join(SIG)  # the plain call's size function serves


@pytest.mark.parametrize("t", [1, 256, 257, 2048, 2049])
def test_the_chunk_length_is_the_kernels_rule(t):
    L = _lib.lib()
    want = 16 * min(max(-(-t // 256), 1), 8)
    assert want == {1: 16, 256: 16, 257: 32, 2048: 128, 2049: 128}[t]
    for d in (16, 48, 128):
        assert L.lqer_attention_q_decode_chunk(t, d) == want == chunk_of(t)


# ---- PageTable.prefix_groups on hand-built tables ---------------------------------------------------------------------------------------
def _table(pages=64, seqs=8, per_seq=32):
    return PageTable(pages, seqs, per_seq)


def _grow(pt, seq, n):
    slots, _, _ = pt.reserve([seq], n)
    pt.commit(slots, n)


def _groups(pt, seqs):
    slots = pt.slots(seqs)
    lens = [pt.lengths[s] for s in slots]
    got = pt.prefix_groups(slots, lens, chunk_of)
    # always a partition: every call index once; members ascending, groups by first member; P a multiple of 16 within every length
    flat = [b for mem, _ in got for b in mem]
    assert sorted(flat) == list(range(len(seqs)))
    assert all(mem == sorted(mem) for mem, _ in got) and [mem[0] for mem, _ in got] == sorted(mem[0] for mem, _ in got)
    for mem, p in got:
        assert p % 16 == 0 and (p == 0) == (len(mem) == 1)
        if p:
            assert all(p <= 16 * (lens[b] // 16) for b in mem) and len({chunk_of(lens[b]) for b in mem}) == 1 and p >= chunk_of(lens[mem[0]])
            assert len({tuple(pt.table[slots[b]][:p // 16]) for b in mem}) == 1  # the same pages
    return got


def _forked(pt, at, kids=2):
    parent = pt.alloc()
    _grow(pt, parent, at)
    return [parent] + pt.fork([parent] * kids)[0]


def test_groups_a_fork_at_37_shares_two_pages():
    pt = _table()
    seqs = _forked(pt, 37)
    assert _groups(pt, seqs) == [([0, 1, 2], 32)]
    for s in seqs:  # one own key each: nothing changes
        _grow(pt, s, 1)
    assert _groups(pt, seqs) == [([0, 1, 2], 32)]
    assert _groups(pt, seqs[::-1]) == [([0, 1, 2], 32)]
    assert _groups(pt, seqs[1:2]) == [([0], 0)]  # alone in the call


def test_groups_a_fork_at_15_shares_no_page():
    pt = _table()
    seqs = _forked(pt, 15)
    for s in seqs:
        _grow(pt, s, 20)  # 35 keys each, pages of their own throughout
    assert _groups(pt, seqs) == [([0], 0), ([1], 0), ([2], 0)]
    assert _groups(pt, _forked(pt, 9)) == [([0], 0), ([1], 0), ([2], 0)]  # below one page: not eligible at all


def test_groups_an_append_across_a_page_boundary_still_shares_the_old_pages_only():
    pt = _table()
    seqs = _forked(pt, 37)
    _grow(pt, seqs[1], 30)  # 67 keys: the pages of keys 32 .. 79 are its own
    _grow(pt, seqs[0], 12)  # 49: across the boundary at 48
    assert [pt.length(s) for s in seqs] == [49, 67, 37]
    assert _groups(pt, seqs) == [([0, 1, 2], 32)]
    # a fork at a page boundary: all 48 keys are shared, and a member that stops there caps nothing below them
    more = _forked(pt, 48)
    _grow(pt, more[2], 5)
    assert _groups(pt, more) == [([0, 1, 2], 48)]


def test_groups_members_of_different_chunk_lengths_part():
    pt = _table()
    seqs = _forked(pt, 240, kids=3)
    _grow(pt, seqs[0], 10)   # 250: C = 16
    _grow(pt, seqs[1], 30)   # 270: C = 32
    _grow(pt, seqs[2], 16)   # 256: C = 16
    _grow(pt, seqs[3], 60)   # 300: C = 32
    assert [chunk_of(pt.length(s)) for s in seqs] == [16, 32, 16, 32]
    assert _groups(pt, seqs) == [([0, 2], 240), ([1, 3], 240)]


def test_groups_dissolve_when_the_shared_keys_are_below_one_chunk():
    pt = _table(pages=128, seqs=4, per_seq=40)
    seqs = _forked(pt, 16)
    for s in seqs:
        _grow(pt, s, 300)  # 316 keys: C = 32, one shared page
    assert _groups(pt, seqs) == [([0], 0), ([1], 0), ([2], 0)]


def test_groups_a_member_with_released_pages_is_alone():
    pt = _table()
    seqs = _forked(pt, 37)
    assert pt.release(seqs[1], 16) == [] and pt.released[pt.slot(seqs[1])] == 1  # (the page lives on: two owners left)
    assert _groups(pt, seqs) == [([0, 2], 32), ([1], 0)]
    pt.release(seqs[2], 32)
    assert _groups(pt, seqs) == [([0], 0), ([1], 0), ([2], 0)]


def test_groups_interleaved_with_strangers_take_the_lowest_call_index_as_leader():
    pt = _table(seqs=9)
    a = _forked(pt, 37)
    b = _forked(pt, 64)
    lone, tiny = pt.alloc(), pt.alloc()
    _grow(pt, lone, 50), _grow(pt, tiny, 9)
    call = [tiny, b[2], a[1], lone, b[0], a[2], a[0], b[1]]
    assert _groups(pt, call) == [([0], 0), ([1, 4, 7], 64), ([2, 5, 6], 32), ([3], 0)]
    # one level: a fork of a fork shares more with its parent than the whole cluster does, and still gets the cluster's keys
    _grow(pt, a[1], 27)  # 64 keys
    grand = pt.fork([a[1]])[0][0]
    assert _groups(pt, [a[0], a[1], grand]) == [([0, 1, 2], 32)]
    assert _groups(pt, [a[1], grand]) == [([0, 1], 64)]


# ---- the call builder -----------------------------------------------------------------------------------------------------------------
def _host_cache():
    """test_kv_paged_call_cpu's host cache - buffers in host memory, launches that do nothing - with a parent of 37 keys, two forks
    and a stranger of 20."""
    import json

    from lqer_amd import PagedKVCache

    with open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")) as fh:
        cfg = json.load(fh)
    cache = PagedKVCache(16, 6, 2, 16, cfg, cfg, torch.float16, "cpu", max_pages_per_seq=16)
    cache._launch_append = cache._launch_fork = lambda *a: None
    z = lambda n: torch.zeros(1, 2, n, 16, dtype=torch.float16)
    parent, lone = cache.alloc(), cache.alloc()
    cache.append([parent], z(37), z(37))
    cache.append([lone], z(20), z(20))
    kids = cache.fork(parent, 2)
    return cache, [kids[0], lone, parent, kids[1]]


def test_the_builder_names_the_shared_entry_with_the_group_arrays():
    cache, seqs = _host_cache()
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    assert lens == [37, 20, 37, 37]
    groups = cache.pt.prefix_groups(slots, lens, chunk_of)
    assert groups == [([0, 2, 3], 32), ([1], 0)]
    q = torch.zeros(4, 4, 3, 16, dtype=torch.float16)
    out = torch.empty_like(q)
    name, args = kvcache._paged_args(kvcache.PAGED_DECODE, q, out, None, cache, slots, lens, 0.25, True, None, 0, 0, None, S=3, groups=groups)
    assert name == SHARED == kvcache.SHARED_DECODE
    assert len(args) == len(SIG[SHARED][1])
    for t, a in zip(SIG[SHARED][1], args):
        t.from_param(a)
    got = dict(zip(_names(SHARED), args))
    plain_name, plain = kvcache._paged_args(kvcache.PAGED_DECODE, q, out, None, cache, slots, lens, 0.25, True, None, 0, 0, None, S=3)
    assert plain_name == PLAIN and len(plain) == len(args) - 5
    for a, b in zip(args, plain):  # the plain call's list in front (ctypes arrays and byref objects by type)
        assert a == b if isinstance(a, (int, float, type(None))) else type(a) is type(b)
    assert got["n_groups"] == 2 and got["batch"] == 4 and got["max_len"] == 256 and got["S"] == 3
    base, g = cache._groups.data_ptr(), cache._groups
    at = {k: (got[k] - base) // 4 for k in ("grp_of", "grp_starts", "grp_members", "grp_keys")}
    assert at == dict(grp_of=0, grp_starts=4, grp_members=7, grp_keys=11)
    assert g[0:4].tolist() == [0, 1, 0, 0] and g[4:7].tolist() == [0, 3, 4] and g[7:11].tolist() == [0, 2, 3, 1] and g[11:13].tolist() == [32, 0]


def test_the_builder_names_the_plain_entry_without_a_group():
    cache, seqs = _host_cache()
    for call in (seqs[:2], seqs[1:2]):  # a fork beside a stranger; the stranger alone
        slots = cache.pt.slots(call)
        lens = [cache.pt.lengths[x] for x in slots]
        groups = cache.pt.prefix_groups(slots, lens, chunk_of)
        assert all(len(mem) == 1 for mem, _ in groups)
        q = torch.zeros(len(call), 4, 1, 16, dtype=torch.float16)
        name, args = kvcache._paged_args(kvcache.PAGED_DECODE, q, q, None, cache, slots, lens, 0.25, False, None, 0, 0, None, S=1, groups=groups)
        assert name == PLAIN and len(args) == len(SIG[PLAIN][1])
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    groups = cache.pt.prefix_groups(slots, lens, chunk_of)
    q = torch.zeros(4, 4, 1, 16, dtype=torch.float16)
    with pytest.raises(ValueError):  # the builder has no windowed or prefill entry with groups
        kvcache._paged_args(kvcache.PAGED_DECODE, q, q, None, cache, slots, lens, 0.25, True, 64, 0, 0, None, S=1, groups=groups)
    with pytest.raises(ValueError):
        kvcache._paged_args(kvcache.PAGED_PREFILL, q, q, None, cache, slots, lens, 0.25, True, None, 0, 0, None, S=1, groups=groups)


def test_python_refuses_a_window_and_the_prefill_kernel():
    cache, seqs = _host_cache()
    q = torch.zeros(4, 4, 1, 16, dtype=torch.float16)
    for kw in (dict(window=64, causal=True), dict(kernel="prefill"), dict(kernel="auto", q=torch.zeros(4, 4, 9, 16, dtype=torch.float16))):
        with pytest.raises(ValueError, match="shared_prefix"):
            attention_flexible_paged(kw.pop("q", q), cache, seqs, 0.25, shared_prefix=True, **kw)
    cache.window = 64  # the cache's window is in effect for a causal call
    with pytest.raises(ValueError, match="shared_prefix"):
        attention_flexible_paged(q, cache, seqs, 0.25, causal=True, shared_prefix=True)


# ---- the library's refusals ---------------------------------------------------------------------------------------------------------------
def _attend(q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
            out=0x40000, ws=0x50000, ws_bytes=1 << 22, batch=3, heads=4, kv=4, S=1, D=64, causal=0, dtype=_lib.F16, of=0x500000, starts=0x500100,
            members=0x500200, keys=0x500300, n_groups=2):
    L = _lib.lib()
    f = _fmt()
    st = (C.c_int64 * 3)(heads * S * D, S * D, D)
    rc = L.lqer_attention_q_decode_paged_shared(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, dtype, batch, heads,
                                                kv, S, D, st, st, 0.125, causal, C.byref(f), C.byref(f), C.byref(f), C.byref(f), ws, ws_bytes, None,
                                                of, starts, members, keys, n_groups)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("null grp_of", dict(of=None), E_INVALID),
    ("null grp_starts", dict(starts=None), E_INVALID),
    ("null grp_members", dict(members=None), E_INVALID),
    ("null grp_keys", dict(keys=None), E_INVALID),
    ("n_groups = 0", dict(n_groups=0), E_INVALID),
    ("negative n_groups", dict(n_groups=-1), E_INVALID),
    ("n_groups > batch", dict(n_groups=4), E_INVALID),
    ("batch = 0 has no group count", dict(batch=0, n_groups=1), E_INVALID),
    # what lqer_attention_q_decode_paged refuses
    ("S = 9", dict(S=9), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("null q", dict(q=None), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("short workspace", dict(ws_bytes=_lib.lib().lqer_attention_q_decode_paged_workspace_bytes(3, 4, 4, 1, 64, 64) - 1), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("max_len beyond the table", dict(max_len=65), E_INVALID),
    ("short pool", dict(pool_bytes=1024), E_INVALID),
    ("batch > 65535", dict(batch=65536, n_groups=1), E_UNSUPPORTED),
])
def test_c_refusals_before_anything_is_launched(case, kwargs, want):
    rc, msg = _attend(**kwargs)
    assert rc == want, (case, rc, msg)
    assert msg.startswith("attention_q_decode_paged_shared:"), msg
    if case == "short workspace":
        assert "lqer_attention_q_decode_paged_workspace_bytes" in msg  # the size function that exists

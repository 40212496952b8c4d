"""A shared prefix read once per group by the decode attention over the paged KV pool, on the GPU (lqer_attention_q_decode_paged_shared:
the GRP instantiation of k_attn_dec_scores / k_attn_dec_pv in csrc/attn_decode.hip; attention_flexible_paged(..., shared_prefix=True),
PageTable.prefix_groups).

The contract is an equality of bits, row for row: out and row_stats of the grouped call are those of the SAME call with
shared_prefix=False, and - per sequence - those of the decode kernel on that sequence's raw K and V alone (attention_flexible with
batch 1: never the paged code itself).  Every comparison is torch.equal on the bytes; there is no tolerance in this file.

Shapes: heads 4, kv heads 2 (R = rep S = 2 S rows per kv head); d 48 in the three dtypes, d 16 and d 128 in fp16.  Fork lengths
  16    one page = one chunk of 16: the whole shared prefix is chunk 0;
  37    chunks 0 and 1 shared, chunk 2 (keys 32 .. 47) mixed: the parent's and every child's own page;
  261   chunks of 32: eight shared chunks of 256 shared keys;
  2100  chunks of 128: 16 shared chunks, and the 17th not shared because 2096 < 2176."""
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_fork as FK
import test_gpu_kv_paged as P
from test_kv_paged_call_cpu import _names

pytestmark = pytest.mark.gpu

CFG, DEV = F.CFG, F.DEV
H, HK, FORMS, FORM_IDS = FK.H, FK.HK, FK.FORMS, FK.FORM_IDS
u8, pages_of = P.u8, P.pages_of
SHARED, PLAIN = "lqer_attention_q_decode_paged_shared", "lqer_attention_q_decode_paged"


class _Entries:
    """The library entries that attention_flexible_paged's builder names while the block runs."""

    def __enter__(self):
        from lqer_amd import kvcache

        self.names, self.kv, self.real = [], kvcache, kvcache._paged_args

        def spy(*a, **kw):
            name, args = self.real(*a, **kw)
            self.names.append(name)
            return name, args

        kvcache._paged_args = spy
        return self.names

    def __exit__(self, *exc):
        self.kv._paged_args = self.real


def _ref(q1, raw, causal):
    """The comparator: the decode kernel on ONE sequence's raw K and V."""
    return P._want(q1, raw[0], raw[1], causal)


def _check(cache, seqs, raws, q, causal, want_groups, what=""):
    """The grouped call against the plain call and against the raw tensors, out and row_stats, for every sequence."""
    from lqer_amd import _lib, attention_flexible_paged

    sc = q.shape[3] ** -0.5
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    groups = cache.pt.prefix_groups(slots, lens, lambda t: _lib.lib().lqer_attention_q_decode_chunk(t, q.shape[3]))
    assert groups == want_groups, f"{what} groups {groups}"
    # (a workspace of 0xFF - NaN in every cell: a cell the grouped call left to nobody shows)
    n, h, s, d = q.shape
    ws = torch.full((_lib.lib().lqer_attention_q_decode_paged_workspace_bytes(n, h, cache.kv_heads, s, cache.pt.max_len, d),), 0xFF, dtype=torch.uint8,
                    device=DEV)
    with _Entries() as names:
        out, st = attention_flexible_paged(q, cache, seqs, sc, causal=causal, return_stats=True, shared_prefix=True, ws=ws)
        plain, plain_st = attention_flexible_paged(q, cache, seqs, sc, causal=causal, return_stats=True)
    assert names == [SHARED if any(len(m) > 1 for m, _ in want_groups) else PLAIN, PLAIN]
    assert torch.equal(u8(out), u8(plain)), f"{what} {(out != plain).sum().item()} outputs differ from the plain call"
    assert torch.equal(u8(st), u8(plain_st)), f"{what} row_stats differ from the plain call"
    for b, raw in enumerate(raws):
        want, want_st = _ref(q[b:b + 1], raw, causal)
        assert torch.equal(u8(out[b:b + 1]), u8(want)), f"{what} sequence {b} ({raw[0].shape[2]} keys): {(out[b:b + 1] != want).sum().item()} outputs differ"
        assert torch.equal(u8(st[b:b + 1]), u8(want_st)), f"{what} sequence {b} ({raw[0].shape[2]} keys): row_stats differ"
    assert torch.isfinite(out).all()
    return out, st


def _forked(cache, prefix, n_kids, tails, seed, d, dtype):
    """A parent appended `prefix`, n_kids forks, then everyone's own keys in append pieces of tails[i]: (seqs, raws)."""
    lp = prefix[0].shape[2]
    parent = cache.alloc()
    cache.append([parent], *prefix)
    seqs = [parent] + cache.fork(parent, n_kids)
    raws = []
    for i, p in enumerate(tails):
        k, v = FK._raw(sum(p), d, dtype, seed + i)
        raws.append((torch.cat([prefix[0], k], 2), torch.cat([prefix[1], v], 2)))
    FK._feed(cache, seqs, raws, tails, [lp] * len(seqs))
    return seqs, raws


# ---- 1. forks at 16, 37, 261, 2100 keys, then diverging tails --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _diverged(dtype, d, lp):
    pats = FK._tails(lp)
    room = pages_of(lp + 40)
    cache = FK._pool(3 * room, 3, d, dtype, room)
    seqs, raws = _forked(cache, FK._raw(lp, d, dtype, 11000 + lp), 2, pats, 11100 + 3 * lp, d, dtype)
    return cache, seqs, raws


@pytest.mark.parametrize("s, causal", [(1, False), (3, True)], ids=["s1", "s3-causal"])
@pytest.mark.parametrize("lp", [16, 37, 261, 2100])
@pytest.mark.parametrize("dtype, d", FORMS, ids=FORM_IDS)
def test_bits_after_a_fork(dtype, d, lp, s, causal):
    from lqer_amd import _lib

    cache, seqs, raws = _diverged(dtype, d, lp)
    lens = [cache.length(x) for x in seqs]
    assert cache.pages_shared == lp // 16 and all(lp < t <= lp + 24 for t in lens)
    C = _lib.lib().lqer_attention_q_decode_chunk(lens[0], d)
    p = 16 * (lp // 16)
    assert (lp, C, p // C, -(-lens[0] // C)) in [(16, 16, 1, 3), (37, 16, 2, 4), (261, 32, 8, 9), (2100, 128, 16, 17)]  # chunk, shared chunks, chunks
    q = F._randn((3, H, s, d), dtype, 110 + s, 3.0).to(DEV)
    _check(cache, seqs, raws, q, causal, [([0, 1, 2], p)], what=f"fork at {lp}:")


# ---- 2. 17 members: 102 rows per kv head, four 32-row groups with members across their boundaries --------------------------------------
def test_seventeen_members():
    dtype, d, lp, n = torch.float16, 48, 37, 17
    cache = FK._pool(2 + 2 * n, n, d, dtype, 4)
    seqs, raws = _forked(cache, FK._raw(lp, d, dtype, 12000), n - 1, [[1 + i % 3] for i in range(n)], 12100, d, dtype)
    assert len(seqs) == n and H // HK * 3 * n == 102
    q = F._randn((n, H, 3, d), dtype, 120, 3.0).to(DEV)
    _check(cache, seqs, raws, q, True, [(list(range(n)), 32)], what="17 members:")
    order = [5, 16, 0, 9, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15]  # another leader, other members at the 32-row boundaries
    _check(cache, [seqs[i] for i in order], [raws[i] for i in order], q, True, [(list(range(n)), 32)], what="17 members, reordered:")


# ---- 3. two groups, a stranger and a short sequence in one call, interleaved -----------------------------------------------------------
@pytest.mark.parametrize("s, causal", [(1, False), (3, True)], ids=["s1", "s3-causal"])
def test_two_groups_and_strangers_interleaved(s, causal):
    dtype, d = torch.float16, 48
    cache = FK._pool(80, 7, d, dtype, 20)
    a, a_raw = _forked(cache, FK._raw(256, d, dtype, 13000), 2, [[24], [44], [1] * 3], 13100, d, dtype)  # 280, 300, 259 keys: chunks of 32
    b, b_raw = _forked(cache, FK._raw(37, d, dtype, 13001), 1, [[3], [1] * 9], 13200, d, dtype)          # 40, 46 keys: chunks of 16
    lone, tiny = cache.alloc(), cache.alloc()
    lone_raw, tiny_raw = FK._raw(50, d, dtype, 13300), FK._raw(9, d, dtype, 13301)
    cache.append([lone], *lone_raw), cache.append([tiny], *tiny_raw)
    assert [cache.length(x) for x in a] == [280, 300, 259] and [cache.length(x) for x in b] == [40, 46]
    seqs = [tiny, b[1], a[1], lone, a[2], b[0], a[0]]
    raws = [tiny_raw, b_raw[1], a_raw[1], lone_raw, a_raw[2], b_raw[0], a_raw[0]]
    q = F._randn((7, H, s, d), dtype, 130 + s, 3.0).to(DEV)
    _check(cache, seqs, raws, q, causal, [([0], 0), ([1, 5], 32), ([2, 4, 6], 256), ([3], 0)], what="two groups:")


# ---- 4. the C call itself: P as a licence, groups of one, guard zones, a pool that is only read -----------------------------------------
def _c_call(cache, seqs, q, out, st, causal, groups, ws):
    """lqer_attention_q_decode_paged_shared with the given groups, whatever they are (the builder would hand groups of one to the
    plain entry)."""
    from lqer_amd import _lib, kvcache, ops

    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    name, args = kvcache._paged_args(kvcache.PAGED_DECODE, q, out, st, cache, slots, lens, q.shape[3] ** -0.5, causal, None, ws.data_ptr(), ws.numel(),
                                     ops._stream(q.device), S=q.shape[2])
    assert name == PLAIN
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().lqer_attention_q_decode_paged_shared(*args, *cache._call_groups(groups)), SHARED)


@pytest.mark.parametrize("groups", [[([0, 1, 2], 32), ([3], 0)], [([0, 1, 2], 16), ([3], 0)], [([1, 0, 2], 32), ([3], 0)], [([0, 2], 32), ([1], 0), ([3], 0)],
                                    [([0], 0), ([1], 0), ([2], 0), ([3], 0)], [([0, 1, 2], 0), ([3], 0)]],
                         ids=["P32", "P16-of-32", "leader-1", "two-of-three", "singletons", "P0"])
def test_c_call_groups_are_a_licence_and_nothing_outside_is_written(groups):
    from lqer_amd import PagedKVCache, _lib

    dt, d, s, stride = torch.float16, 48, 3, 4
    cache = PagedKVCache(12, 4, HK, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=0xFF, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(4, stride)
    seqs, raws = _forked(cache, FK._raw(37, d, dt, 14000), 2, [[2], [5], [9]], 14100, d, dt)
    lone, lone_raw = cache.alloc(), FK._raw(21, d, dt, 14200)
    cache.append([lone], *lone_raw)
    seqs, raws = seqs + [lone], raws + [lone_raw]
    n = len(seqs)
    g_q = _guard.guarded(n * H * s * d * 2, align=16, name="q").load(F._randn((n, H, s, d), dt, 140, 3.0).to(DEV))
    q = g_q.view(dt).view(n, H, s, d)
    need = _lib.lib().lqer_attention_q_decode_paged_workspace_bytes(n, H, HK, s, cache.pt.max_len, d)
    g_ws = _guard.guarded(need, align=16, fill=0xFF, name="workspace")
    g_out = _guard.guarded(n * H * s * d * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(n * H * s * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(n, H, s, d), g_st.view(torch.float32).view(n, H, s, 2)
    torch.cuda.synchronize()
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    _c_call(cache, seqs, q, out, st, True, groups, g_ws.payload)
    torch.cuda.synchronize()
    g_ws.check(), g_out.check(), g_st.check(), g_pool.check(), g_tbl.check(), g_q.unchanged()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)  # the pool is only read
    for b, raw in enumerate(raws):
        want, want_st = _ref(q[b:b + 1], raw, True)
        assert torch.equal(u8(out[b:b + 1]), u8(want)) and torch.equal(u8(st[b:b + 1]), u8(want_st)), f"groups {groups}: sequence {b} differs"


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """The three launches captured once on one stream (no parallel branches) and replayed: the eager call's bits, for new queries too."""
    from lqer_amd import _lib, kvcache, ops

    dtype, d, s = torch.float16, 48, 3
    cache = FK._pool(12, 3, d, dtype, 4)
    seqs, raws = _forked(cache, FK._raw(37, d, dtype, 15000), 2, [[1], [2], [3]], 15100, d, dtype)
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    L = _lib.lib()
    groups = cache.pt.prefix_groups(slots, lens, lambda t: L.lqer_attention_q_decode_chunk(t, d))
    assert groups == [([0, 1, 2], 32)]
    q = F._randn((3, H, s, d), dtype, 150, 3.0).to(DEV)
    out = torch.empty_like(q)
    st = torch.empty(3, H, s, 2, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.lqer_attention_q_decode_paged_workspace_bytes(3, H, HK, s, cache.pt.max_len, d), dtype=torch.uint8, device=DEV)
    # the metadata goes up before the capture; the recorded call takes the capture's stream
    name, args = kvcache._paged_args(kvcache.PAGED_DECODE, q, out, st, cache, slots, lens, d ** -0.5, True, None, ws.data_ptr(), ws.numel(), None, S=s,
                                     groups=groups)
    assert name == SHARED
    at = _names(SHARED).index("stream")
    call = lambda: _lib.check(getattr(L, name)(*args[:at], ops._stream(q.device), *args[at + 1:]), name)
    call()
    torch.cuda.synchronize()
    eager, eager_st = out.clone(), st.clone()
    for b, raw in enumerate(raws):
        want, want_st = _ref(q[b:b + 1], raw, True)
        assert torch.equal(u8(eager[b:b + 1]), u8(want)) and torch.equal(u8(eager_st[b:b + 1]), u8(want_st))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seed in (150, 151):
        q.copy_(F._randn((3, H, s, d), dtype, seed, 3.0).to(DEV))
        out.fill_(0), st.fill_(0), ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        if seed == 150:
            assert torch.equal(u8(out), u8(eager)) and torch.equal(u8(st), u8(eager_st))
        else:
            assert not torch.equal(u8(out), u8(eager))
            for b, raw in enumerate(raws):
                want, want_st = _ref(q[b:b + 1], raw, True)
                assert torch.equal(u8(out[b:b + 1]), u8(want)) and torch.equal(u8(st[b:b + 1]), u8(want_st))


# ---- 6. a shared chunk is read through the leader's table row alone ------------------------------------------------------------------------
@pytest.mark.parametrize("lp", [37, 1029])
def test_a_shared_chunk_is_loaded_through_the_leaders_row(lp):
    """The other members' table entries below the last shared chunk's end point at the pages of a STRANGER (valid pages, other keys):
    the grouped call still gives every member its bits - nothing of a shared chunk is read through a member's own row -, the entries
    of the chunks that are not shared (the rest of the licence P included) are read as ever, and the plain call on that table gives
    the members other bits, so the check can fail.  37 keys: chunks of 16; 1029: chunks of 80, 12 of them below P = 1024."""
    from lqer_amd import _lib

    dt, d, s = torch.float16, 48, 3
    room = pages_of(lp + 16)
    cache = FK._pool(3 * room + room, 4, d, dt, room)
    seqs, raws = _forked(cache, FK._raw(lp, d, dt, 16000 + lp), 2, [[1], [2], [3]], 16100 + lp, d, dt)
    lone, lone_raw = cache.alloc(), FK._raw(lp, d, dt, 16200 + lp)
    cache.append([lone], *lone_raw)
    C = _lib.lib().lqer_attention_q_decode_chunk(lp + 1, d)
    p = 16 * (lp // 16)
    below = p // C * C // 16  # table entries of the shared chunks
    assert (C, below) == {37: (16, 2), 1029: (80, 60)}[lp] and below <= p // 16
    row = torch.tensor(cache.pt.table[cache.pt.slot(lone)][:below], dtype=torch.int32, device=DEV)
    for x in seqs[1:]:
        cache.table[cache.pt.slot(x), :below] = row  # (the device table only: the books, and with them the groups, stay)
    q = F._randn((3, H, s, d), dt, 160, 3.0).to(DEV)
    out, st = torch.empty_like(q), torch.empty(3, H, s, 2, dtype=torch.float32, device=DEV)
    ws = torch.full((_lib.lib().lqer_attention_q_decode_paged_workspace_bytes(3, H, HK, s, cache.pt.max_len, d),), 0xFF, dtype=torch.uint8, device=DEV)
    _c_call(cache, seqs, q, out, st, True, [([0, 1, 2], p)], ws)
    for b, raw in enumerate(raws):
        want, want_st = _ref(q[b:b + 1], raw, True)
        assert torch.equal(u8(out[b:b + 1]), u8(want)) and torch.equal(u8(st[b:b + 1]), u8(want_st)), f"fork at {lp}: sequence {b} differs"
    _c_call(cache, seqs, q, out, st, True, [([0], 0), ([1], 0), ([2], 0)], ws)  # groups of one: every sequence through its own row
    want, want_st = _ref(q[:1], raws[0], True)
    assert torch.equal(u8(out[:1]), u8(want)) and torch.equal(u8(st[:1]), u8(want_st))
    for b in (1, 2):
        assert not torch.equal(u8(out[b:b + 1]), u8(_ref(q[b:b + 1], raws[b], True)[0])), "the stranger's pages changed nothing"

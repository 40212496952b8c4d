"""Per-sequence query counts on the split decode kernels of the paged KV pool, on the GPU (lqer_attention_q_decode_paged_ragged: the
ragged instantiation of k_attn_dec_scores / k_attn_dec_pv / k_attn_dec_sum of csrc/attn_decode.hip, with and without the window rule;
attention_flexible_paged_decode_ragged, attention_flexible_paged_ragged(kernel="auto")).

The contract is an equality of bits per sequence: the rows of sequence b in out and row_stats of one call over sequences with counts
of their own are those of the decode kernel on the raw K and V of that sequence alone with S = counts[b] -
attention_flexible(q_b, K_b, V_b, ..., kernel="decode") with batch 1, never the paged code itself; with a window, the same call on the
FULL raw K and V with the additive window mask (test_gpu_kv_window.py's).  Every comparison is torch.equal on the bytes; there is no
tolerance in this file.  Every sequence is at least as long as its own count (causal needs counts[b] <= length_b).

Lengths (8, 15, 16, 17, 33, 255, 256, 257, 2049): a short sequence, the page edge, the chunk rule's step (256: 16 chunks of 16; 257: 9 of
32) and 17 chunks of 128.  7 rows on the 8 keys put the first query row at position 1: it sees keys 0 and 1 only.
Head geometries: d 48, heads 4 / 2 (d no multiple of 32); d 128, heads 16 / 2 (rep 8: counts 3, 4, 5 and 8 are 24, 32, 40 and 64 rows per
kv head, on both sides of the 32-row group); d 64, heads 8 / 8.
Count sets: every count of 1 .. 8 in one call; (1, 8, 0, 3, 5); every count 1."""
import ctypes as C
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
from test_gpu_kv_paged import _pool_spans, pages_of, u8
from test_gpu_kv_ragged import _padded, starts_of
from test_gpu_kv_window import _mask

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES = F.CFG, F.DEV, F.DTYPES
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
F16 = torch.float16
LENS = (8, 15, 16, 17, 33, 255, 256, 257, 2049)
GEOM = {"d48": (48, 4, 2), "d128": (128, 16, 2), "d64": (64, 8, 8)}  # d, heads, kv heads
# name -> (the indices into LENS of the call's sequences, their counts)
COUNTS = {"all": (tuple(range(9)), (7, 8, 1, 2, 3, 4, 5, 6, 8)),   # 7 rows on 8 keys; 8 rows on 15 and on 2049; 5 rows on 256, 6 on 257
          "mixed": ((7, 8, 2, 0, 5), (1, 8, 0, 3, 5)),              # 257, 2049, 16 (left out), 8 and 255 keys
          "ones": (tuple(range(9)), (1,) * 9)}
BEYOND = 4096  # a window beyond every length: plain causal


@functools.lru_cache(maxsize=None)
def _raw(geom, dtype):
    """The raw K and V of the nine sequences, [1, hk, L, d] each, on the device: made once, shared, never written."""
    d, _, hk = GEOM[geom]
    return tuple(tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dtype, 7000 + 16 * i + d, 2.0)) for i, n in enumerate(LENS))


@functools.lru_cache(maxsize=None)
def _pool(geom, dtype):
    """The nine sequences in a cache without a window (every page kept), each appended with one call: (cache, seqs)."""
    from lqer_amd import PagedKVCache

    d, _, hk = GEOM[geom]
    cache = PagedKVCache(sum(map(pages_of, LENS)), len(LENS), hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=max(map(pages_of, LENS)))
    seqs = [cache.alloc() for _ in LENS]
    for s, (k, v) in zip(seqs, _raw(geom, dtype)):
        cache.append([s], k, v)
    return cache, seqs


@functools.lru_cache(maxsize=None)
def _q1(geom, dtype, i, c):
    """The c query rows of sequence i, [1, h, c, d]."""
    d, h, _ = GEOM[geom]
    return F._randn((1, h, c, d), dtype, 300 + 16 * i + c, 3.0).to(DEV)


def _rows(out, st):
    return out[0].transpose(0, 1).contiguous(), st[0].transpose(0, 1).contiguous()


def _compare(q1, k, v, causal, w=None):
    """The comparator on ONE sequence's raw tensors: the decode kernel, as rows [c, h, d] and [c, h, 2]."""
    from lqer_amd import attention_flexible

    kw = dict(causal=causal) if w is None else dict(attention_mask=_mask(k.shape[2], q1.shape[2], w, q1.dtype))
    return _rows(*attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, kernel="decode", return_stats=True, **kw))


@functools.lru_cache(maxsize=None)
def _want(geom, dtype, i, c, causal, w=None):
    """The comparator for sequence i with c query rows (w: the window as a mask tensor on the full K and V).  Made once, never written."""
    k, v = _raw(geom, dtype)[i]
    return _compare(_q1(geom, dtype, i, c), k, v, causal, w)


def _queries(geom, dtype, pick, counts):
    return torch.cat([_q1(geom, dtype, i, c)[0].transpose(0, 1) for i, c in zip(pick, counts) if c]).contiguous()


def _check(geom, dtype, pick, counts, causal, out, st, w=None, what=""):
    at = starts_of(counts)
    for b, (i, c) in enumerate(zip(pick, counts)):
        if not c:
            continue
        want, want_st = _want(geom, dtype, i, c, causal, w)
        got, got_st = out[at[b]:at[b + 1]], st[at[b]:at[b + 1]]
        assert got.shape == want.shape and got_st.shape == want_st.shape
        assert torch.equal(u8(got), u8(want)), f"{what} sequence {i} ({LENS[i]} keys, {c} rows, window {w}): {(got != want).sum().item()} outputs differ"
        assert torch.equal(u8(got_st), u8(want_st)), f"{what} sequence {i} ({LENS[i]} keys, {c} rows, window {w}): row_stats differ"


# ---- 1. bits per sequence ----------------------------------------------------------------------------------------------------------
CASES1 = [(g, dt, causal, cs) for g in GEOM for dt in DTYPES for causal in (False, True) for cs in COUNTS]


@pytest.mark.parametrize("geom, dtype, causal, cs", CASES1, ids=[f"{g}-{DT_ID[dt]}-{'causal' if c else 'full'}-{cs}" for g, dt, c, cs in CASES1])
def test_bits_per_sequence(geom, dtype, causal, cs):
    from lqer_amd import attention_flexible_paged_decode_ragged

    cache, seqs = _pool(geom, dtype)
    pick, counts = COUNTS[cs]
    q = _queries(geom, dtype, pick, counts)
    out, st = attention_flexible_paged_decode_ragged(q, cache, [seqs[i] for i in pick], counts, q.shape[2] ** -0.5, causal=causal, return_stats=True)
    assert out.shape == q.shape and out.dtype == q.dtype and st.shape == (*q.shape[:2], 2) and st.dtype == torch.float32
    _check(geom, dtype, pick, counts, causal, out, st)
    assert torch.isfinite(out).all()
    alone = attention_flexible_paged_decode_ragged(q, cache, [seqs[i] for i in pick], counts, q.shape[2] ** -0.5, causal=causal)  # (without the statistics)
    assert torch.equal(u8(alone), u8(out))


def test_the_sets_reach_the_edges_they_are_there_for():
    """Host arithmetic of the kernels' rules."""
    chunk = lambda t: 16 * min(max((t + 255) // 256, 1), 8)
    nch = lambda t: -(-t // chunk(t))
    lo = lambda t, s, w: max(0, t - s - w + 1)
    assert [nch(t) for t in LENS] == [1, 1, 1, 2, 3, 16, 16, 9, 17]       # the non-monotonic chunk count; 17 chunks of 128
    pick, counts = COUNTS["all"]
    assert sorted(set(counts)) == list(range(1, 9)) and all(c <= LENS[i] for i, c in zip(pick, counts))
    assert counts[0] == 7 and LENS[0] - 7 == 1                              # the first query row at position 1: keys 0 and 1
    assert {8 * c for c in counts} >= {24, 32, 40, 64}                      # rep 8: both sides of the 32-row group
    assert all(c <= LENS[i] for i, c in zip(*COUNTS["mixed"])) and 0 in COUNTS["mixed"][1]
    assert chunk(296) == 32 and lo(296, 1, 8) // 32 == 9 and lo(296, 8, 8) // 32 == 8  # equal lengths, different first live chunks
    assert lo(2049, 8, 20) // 128 == 15 and lo(257, 6, 20) // 16 == 14 and lo(8, 7, 1) == 1


# ---- 2. the window rule ------------------------------------------------------------------------------------------------------------
CASES2 = ([("d48", dt, w, cs) for dt in DTYPES for w in (1, 8, 20, BEYOND) for cs in ("all", "mixed")] + [("d128", F16, 20, "all"), ("d64", F16, 8, "all")])


@pytest.mark.parametrize("geom, dtype, w, cs", CASES2, ids=[f"{g}-{DT_ID[dt]}-w{w}-{cs}" for g, dt, w, cs in CASES2])
def test_window_bits_per_sequence(geom, dtype, w, cs):
    from lqer_amd import attention_flexible_paged_decode_ragged

    cache, seqs = _pool(geom, dtype)
    pick, counts = COUNTS[cs]
    q = _queries(geom, dtype, pick, counts)
    out, st = attention_flexible_paged_decode_ragged(q, cache, [seqs[i] for i in pick], counts, q.shape[2] ** -0.5, causal=True, return_stats=True, window=w)
    _check(geom, dtype, pick, counts, True, out, st, w=w)
    assert torch.isfinite(out).all()
    if w == BEYOND:  # plain causal
        plain, plain_st = attention_flexible_paged_decode_ragged(q, cache, [seqs[i] for i in pick], counts, q.shape[2] ** -0.5, causal=True, return_stats=True)
        assert torch.equal(u8(out), u8(plain)) and torch.equal(u8(st), u8(plain_st))


def _kv(n, d, hk, dtype, seed):
    return tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dtype, seed, 2.0))


def test_equal_lengths_take_different_first_live_chunks():
    """Two sequences of 296 keys (chunks of 32), W = 8, counts 1 and 8: lo = 288 and 281, the first live chunks 9 and 8 - a workgroup
    takes its first live chunk from its OWN count; the chunk that writes row_stats differs too."""
    from lqer_amd import PagedKVCache, attention_flexible_paged_decode_ragged

    d, h, hk, dt, w = 48, 4, 2, F16, 8
    raws = [_kv(296, d, hk, dt, 7700 + i) for i in range(2)]
    cache = PagedKVCache(2 * pages_of(296), 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=pages_of(296))
    seqs = [cache.alloc(), cache.alloc()]
    for s, (k, v) in zip(seqs, raws):
        cache.append([s], k, v)
    for counts in ((1, 8), (8, 1)):
        qs = [F._randn((1, h, c, d), dt, 40 + c, 3.0).to(DEV) for c in counts]
        q = torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous()
        out, st = attention_flexible_paged_decode_ragged(q, cache, seqs, counts, d ** -0.5, causal=True, return_stats=True, window=w)
        at = starts_of(counts)
        for b, (k, v) in enumerate(raws):
            want, want_st = _compare(qs[b], k, v, True, w)
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st)), (counts, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
def test_released_pages_are_never_read(dtype):
    """The sequences grow in a cache with W = 20, so their old pages go back to the pool; every free page is then overwritten with a
    byte pattern (0xA5: other codes, large exponents).  The stale entries of the rows name those pages, and the bits still are the
    comparator's on the full raw K and V - for the cache's window and for a narrower one."""
    from lqer_amd import PagedKVCache, attention_flexible_paged_decode_ragged

    w, d, h, hk, lens = 20, 48, 4, 2, (37, 70, 100, 300)
    raws = [_kv(n, d, hk, dtype, 7800 + i) for i, n in enumerate(lens)]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens), hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=pages_of(300), window=w)
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v), step in zip(seqs, raws, (1, 5, 8, 7)):
        for at in range(0, k.shape[2], step):
            cache.append([s], k[:, :, at:at + step], v[:, :, at:at + step])
    gone = [cache.pt.released[cache.pt.slot(s)] for s in seqs]
    assert gone == [max(0, (n - w - 7) // 16) for n in lens] == [0, 2, 4, 17]
    held = {p for s, g in zip(seqs, gone) for p in cache.pt.table[cache.pt.slot(s)][g:cache.pt.pages_of[cache.pt.slot(s)]]}
    stale = {p for s, g in zip(seqs, gone) for p in cache.pt.table[cache.pt.slot(s)][:g]}
    free = set(cache.pt._free_pages)
    assert not free & held and stale - held <= free and stale & free
    torch.cuda.synchronize()
    for lo, hi in _pool_spans(cache, sorted(free), 0)[:-1]:  # (all but the slot's staging rows)
        cache.buf[lo:hi] = 0xA5
    for counts, win, seed in (((1, 8, 3, 5), None, 0), ((8, 1, 2, 7), None, 1), ((2, 5, 8, 1), 9, 2)):
        qs = [F._randn((1, h, c, d), dtype, 60 + 8 * seed + c, 3.0).to(DEV) for c in counts]
        q = torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous()
        out, st = attention_flexible_paged_decode_ragged(q, cache, seqs, counts, d ** -0.5, causal=True, return_stats=True, **({} if win is None else {"window": win}))
        at = starts_of(counts)
        for b, (k, v) in enumerate(raws):
            want, want_st = _compare(qs[b], k, v, True, win or w)
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st)), (counts, win, b)
        assert torch.isfinite(out).all()


# ---- the C call itself: bounds, buffers and a workspace of the caller's ----------------------------------------------------------------
def _c_call(cache, seqs, counts, q, out, st, causal, window=0, max_s=None, max_len=None, total=None, ws=None, ws_fill=0xFF):
    """lqer_attention_q_decode_paged_ragged as it stands: every sequence of the call is handed over, a count of 0 included; q / out
    [rows, h, d] views with any token and head stride."""
    from lqer_amd import _lib, ops
    from lqer_amd.kvcache import _pair

    L, f = _lib.lib(), cache.fmts
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[s] for s in slots]
    h, d = q.shape[1], q.shape[2]
    max_s = max(max(counts), 1) if max_s is None else max_s
    max_len = min((max(max(lens), 1) + 127) // 128 * 128, cache.pt.max_len) if max_len is None else max_len
    total = sum(counts) if total is None else total
    if ws is None:
        ws = torch.full((max(L.lqer_attention_q_decode_paged_ragged_workspace_bytes(total, h, max_len, d), 16),), ws_fill, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(q.device):
        _lib.check(L.lqer_attention_q_decode_paged_ragged(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(),
                                                          st.data_ptr() if st is not None else None, ops.dtype_code(q), len(seqs), h, cache.kv_heads,
                                                          cache._call_starts(counts), max_s, total, d, _pair(q), _pair(out), d ** -0.5, int(causal),
                                                          C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), C.byref(f[3]), ws.data_ptr(), ws.numel(),
                                                          ops._stream(q.device), window), "lqer_attention_q_decode_paged_ragged")


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 20], ids=["causal", "w20"])
def test_rows_do_not_depend_on_the_batch_the_bounds_or_the_buffers(window):
    """d 128, heads 16 / 2.  Sequences 0 (8 keys, 7 rows), 6 (256 keys, 5 rows = 40 rows per kv head) and 8 (2049 keys, 8 rows): alone,
    inside the batch of nine and inside the reversed batch; with max_s tight and at 8; with max_len tight and at the table's room (other
    workspace strides, another grid); from q / out buffers with spare tokens behind `total`, `total` beyond the rows in use and a
    padded token stride; with the workspace pre-filled with 0xFF and with zeros.  Every setting gives the comparator's bits."""
    geom, dt = "d128", F16
    d, h, _ = GEOM[geom]
    cache, seqs = _pool(geom, dt)
    pick_all, counts_all = COUNTS["all"]
    w = window or None
    assert cache.pt.max_len == 2064
    for target in (0, 6, 8):
        for order in ([target], list(pick_all), list(pick_all)[::-1]):
            cs = [counts_all[i] for i in order]
            total, at, b = sum(cs), starts_of(cs), order.index(target)
            want, want_st = (u8(x) for x in _want(geom, dt, target, counts_all[target], True, w))
            q = _queries(geom, dt, order, cs)
            for max_s, max_len in ((None, None), (8, None), (8, cache.pt.max_len)):
                for fill in (0xFF, 0x00):
                    _, qv = _padded(total, h, d, dt, 5, 24, 0xFF)
                    qv.copy_(q)
                    obase, ov = _padded(total, h, d, dt, 5, 8, 0x5A)
                    sv = torch.full((total + 5, h, 2), 7.0, dtype=torch.float32, device=DEV)
                    _c_call(cache, [seqs[i] for i in order], cs, qv, ov, sv, True, window=window, max_s=max_s, max_len=max_len, total=total + 5, ws_fill=fill)
                    assert torch.equal(u8(ov[at[b]:at[b + 1]]), want) and torch.equal(u8(sv[at[b]:at[b + 1]]), want_st), (target, order, max_s, max_len, fill)
                    assert bool((sv[total:] == 7.0).all())
                    keep = torch.ones_like(obase, dtype=torch.bool)
                    keep.as_strided(ov.shape, ov.stride()).fill_(False)
                    assert bool((u8(obase[keep]) == 0x5A).all())  # the spare tokens and the padding of out keep their bytes


# ---- 4. zero counts, empty sequences -------------------------------------------------------------------------------------------------
def test_zero_counts_in_the_c_call_write_nothing():
    """Five sequences handed to the library, one with S_b = 0: its workgroups leave at once, the others' rows are the comparator's, and
    an out filled with a pattern keeps it everywhere else.  Every count 0: nothing at all is written.  A sequence of length 0 WITH a
    count gets zero rows and no statistics, as the uniform entry gives it."""
    from lqer_amd import PagedKVCache

    geom, dt = "d48", F16
    d, h, hk = GEOM[geom]
    cache, seqs = _pool(geom, dt)
    pick, counts = COUNTS["mixed"]
    total = sum(counts)
    q = _queries(geom, dt, pick, counts)
    for window in (0, 8):
        obase, ov = _padded(total, h, d, dt, 3, 16, 0x5A)
        sv = torch.full((total + 3, h, 2), 7.0, dtype=torch.float32, device=DEV)
        _c_call(cache, [seqs[i] for i in pick], counts, q, ov, sv, True, window=window, total=total + 3)
        _check(geom, dt, pick, counts, True, ov, sv[:total], w=window or None)
        keep = torch.ones_like(obase, dtype=torch.bool)
        keep.as_strided(ov.shape, ov.stride()).fill_(False)
        assert bool((u8(obase[keep]) == 0x5A).all()) and bool((sv[total:] == 7.0).all())
        # every count 0: nothing at all is written
        obase.view(torch.uint8).fill_(0x5A)
        sv.fill_(7.0)
        _c_call(cache, [seqs[i] for i in pick], (0,) * 5, q, ov, sv, True, window=window, max_s=1, total=total)
        torch.cuda.synchronize()
        assert bool((u8(obase) == 0x5A).all()) and bool((sv == 7.0).all())
    # lens[b] = 0 with a count of 2 beside a sequence of 20 keys with 3 rows
    small = PagedKVCache(2, 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=2)
    empty, full = small.alloc(), small.alloc()
    k, v = _kv(20, d, hk, dt, 7900)
    small.append([full], k, v)
    q2 = F._randn((1, h, 5, d), dt, 77, 3.0).to(DEV)
    qp = q2[0].transpose(0, 1).contiguous()
    out = torch.full((5, h, d), 3.0, dtype=dt, device=DEV)
    st = torch.full((5, h, 2), 7.0, dtype=torch.float32, device=DEV)
    _c_call(small, [empty, full], (2, 3), qp, out, st, False)
    want, want_st = _compare(q2[:, :, 2:], k, v, False)
    assert bool((out[:2] == 0).all()) and bool((st[:2] == 7.0).all())
    assert torch.equal(u8(out[2:]), u8(want)) and torch.equal(u8(st[2:]), u8(want_st))


# ---- 5. footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 8], ids=["causal", "w8"])
def test_footprint(window):
    """Pool and workspace start at 0xFF; q is a guarded input; out, statistics, workspace, pool and table carry guard zones, and the
    attention writes nothing of the pool or the table."""
    from lqer_amd import PagedKVCache, _lib

    dt, d, h, hk, stride = F16, 48, 4, 2, 4
    cache = PagedKVCache(11, 4, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=0xFF, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(4, stride)
    seqs = [cache.alloc() for _ in range(4)]
    lens, counts = (41, 35, 18, 5), (1, 8, 0, 5)
    raws = [_kv(t, d, hk, dt, 8000 + i) for i, t in enumerate(lens)]
    for s, (k, v) in zip(seqs, raws):
        cache.append([s], k, v)
    total = sum(counts)
    qs = [F._randn((1, h, c, d), dt, 90 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    g_q = _guard.guarded(total * h * d * 2, align=16, name="q").load(torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous())
    max_len = 64
    need = _lib.lib().lqer_attention_q_decode_paged_ragged_workspace_bytes(total, h, max_len, d)
    g_ws = _guard.guarded(need, align=16, fill=0xFF, name="workspace")
    g_out = _guard.guarded(total * h * d * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(total * h * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(total, h, d), g_st.view(torch.float32).view(total, h, 2)
    torch.cuda.synchronize()
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    _c_call(cache, seqs, counts, g_q.view(dt).view(total, h, d), out, st, True, window=window, max_len=max_len, ws=g_ws.payload)
    torch.cuda.synchronize()
    g_ws.check(), g_out.check(), g_st.check(), g_pool.check(), g_tbl.check(), g_q.unchanged()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)
    at = starts_of(counts)
    for b, ((k, v), c) in enumerate(zip(raws, counts)):
        if c:
            want, want_st = _compare(qs[b], k, v, True, window or None)
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st)), b
    assert torch.isfinite(out).all()


# ---- 6. the Python level -------------------------------------------------------------------------------------------------------------
def test_equals_the_uniform_decode_call_on_each_sequence_alone():
    from lqer_amd import attention_flexible_paged, attention_flexible_paged_decode_ragged

    geom, dt = "d64", torch.bfloat16
    d, h, _ = GEOM[geom]
    cache, seqs = _pool(geom, dt)
    for cs, window in (("all", None), ("mixed", None), ("all", 20)):
        pick, counts = COUNTS[cs]
        q = _queries(geom, dt, pick, counts)
        out, st = attention_flexible_paged_decode_ragged(q, cache, [seqs[i] for i in pick], counts, d ** -0.5, causal=True, return_stats=True, window=window)
        at = starts_of(counts)
        for b, (i, c) in enumerate(zip(pick, counts)):
            if c:
                want, want_st = attention_flexible_paged(_q1(geom, dt, i, c), cache, [seqs[i]], d ** -0.5, causal=True, return_stats=True, kernel="decode",
                                                         window=window)
                assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want[0].transpose(0, 1))), (cs, window, i)
                assert torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st[0].transpose(0, 1))), (cs, window, i)


@pytest.mark.parametrize("window", [None, 64], ids=["plain", "w64"])
def test_one_mixed_step_through_auto(window):
    """Counts (1, 1, 3, 8, 1, 33, 2): the six sequences of up to 8 rows in ONE decode call - their rows gathered, the chunk's 33 rows
    lie between them - and the chunk in one prefill call (40 keys: inside the window), on a cache with a window (old pages released on
    the way) and on a plain one.  Every sequence's rows are those attention_flexible_paged(kernel="auto") gives it alone."""
    from lqer_amd import PagedKVCache, attention_flexible_paged, attention_flexible_paged_ragged

    dt, d, h, hk = F16, 64, 8, 2
    lens, counts = (254, 300, 100, 2049, 16, 40, 257), (1, 1, 3, 8, 1, 33, 2)
    raws = [_kv(t, d, hk, dt, 8100 + i) for i, t in enumerate(lens)]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens), hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=max(map(pages_of, lens)), window=window)
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v) in zip(seqs, raws):
        for at in range(0, k.shape[2], 64):
            cache.append([s], k[:, :, at:at + 64], v[:, :, at:at + 64])
    assert (window is None) == (not any(cache.pt.released))
    plan = attention_flexible_paged_ragged.plan(cache, seqs, counts)
    assert [(p["call"], p["seqs"], p["rows"], p["window"]) for p in plan] == [
        ("lqer_attention_q_decode_paged_ragged", [0, 1, 2, 3, 4, 6], "gathered", window), ("lqer_attention_q_paged_ragged", [5], "view", None)]
    qs = [F._randn((1, h, c, d), dt, 130 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    q = torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous()
    out, st = attention_flexible_paged_ragged(q, cache, seqs, counts, d ** -0.5, causal=True, return_stats=True)
    at = starts_of(counts)
    for b, (s, c) in enumerate(zip(seqs, counts)):
        want, want_st = attention_flexible_paged(qs[b], cache, [s], d ** -0.5, causal=True, return_stats=True, kernel="auto")
        assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want[0].transpose(0, 1))) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st[0].transpose(0, 1))), b
        if c <= 8:  # ... and the decode kernel's on the raw tensors
            k, v = raws[b]
            raw, raw_st = _compare(qs[b], k, v, True, window)
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(raw)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(raw_st)), b
    assert torch.isfinite(out).all()

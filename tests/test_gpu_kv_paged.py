"""The paged KV pool on the GPU (lqer_kv_pool_append / lqer_attention_q_decode_paged / lqer_kv_pool_gather; csrc/kv_cache.hip,
csrc/attn_decode.hip with the paged operand source; lqer_amd.kvcache.PagedKVCache, attention_flexible_paged).

The contract is an equality of bits per sequence: out[b] and row_stats[b] of one call over sequences of different lengths are those of
the decode kernel on the raw K and V of sequence b alone (attention_flexible(..., kernel="decode") with batch 1 - never the paged code
itself), and the pool's bytes are those of a dense QuantizedKVCache built from the same raw tensors with the same append pattern.
Every comparison is torch.equal on the bytes; there is no tolerance in this file.

Length sets, the smallest that reach every edge:
  A (1, 15, 16, 17, 37)    D 48, heads 4 / 2: below, at and above one page, and a ragged page;
  B (255, 256, 257, 300)   D 64, heads 8 / 2: the chunk rule's step - 16, 16, 9 and 10 chunks, so the grid has more chunks than the
                           longest sequence owns;
  C (2048, 2049, 5)        D 16, heads 2 / 1: chunks of 128 - 16, 17 and 1 chunks in one grid."""
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES = F.CFG, F.DEV, F.DTYPES
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
SETS = {"A": ((1, 15, 16, 17, 37), 48, 4, 2), "B": ((255, 256, 257, 300), 64, 8, 2), "C": ((2048, 2049, 5), 16, 2, 1)}  # lengths, d, h, hk
pages_of = lambda n: (n + 15) // 16
u8 = lambda t: t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _raw(name, dtype):
    """The raw K and V of the set's sequences, [1, hk, L, d] each, on the device: made once, shared, never written."""
    lens, d, _, hk = SETS[name]
    return tuple(tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dtype, 1000 + 16 * i + ord(name), 2.0)) for i, n in enumerate(lens))


def _build(name, dtype, max_pages_per_seq=None, spare=0):
    """A PagedKVCache with the set's sequences, each appended with one call; the pool has exactly the pages they need (+ spare)."""
    from lqer_amd import PagedKVCache

    lens, d, _, hk = SETS[name]
    cache = PagedKVCache(sum(map(pages_of, lens)) + spare, len(lens), hk, d, CFG, CFG, dtype, DEV,
                         max_pages_per_seq=max_pages_per_seq or max(map(pages_of, lens)))
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v) in zip(seqs, _raw(name, dtype)):
        cache.append([s], k, v)
    assert [cache.length(s) for s in seqs] == list(lens) and cache.pages_free == spare
    return cache, seqs


@functools.lru_cache(maxsize=None)
def _paged(name, dtype):
    return _build(name, dtype)


def _q(name, dtype, n, s, seed=7):
    _, d, h, _ = SETS[name]
    return F._randn((n, h, s, d), dtype, seed + s, 3.0).to(DEV)


def _want(q1, k, v, causal, layout="bhsd"):
    """The comparator: the decode kernel on the raw tensors of ONE sequence."""
    from lqer_amd import attention_flexible

    return attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, causal=causal, kernel="decode", return_stats=True, out_layout=layout)


def _check_bits(cache, seqs, raws, q, causal, layout="bhsd", what=""):
    """out[b] and stats[b] of one paged call over `seqs` against the comparator on raws[b], for every b."""
    from lqer_amd import attention_flexible_paged

    out, st = attention_flexible_paged(q, cache, seqs, q.shape[3] ** -0.5, causal=causal, out_layout=layout, return_stats=True)
    assert out.dtype == q.dtype and st.shape == (*q.shape[:3], 2)
    for b, (k, v) in enumerate(raws):
        want, want_st = _want(q[b:b + 1], k, v, causal, layout)
        assert out[b:b + 1].shape == want.shape
        assert torch.equal(u8(out[b:b + 1]), u8(want)), f"{what} sequence {b} ({k.shape[2]} keys): {(out[b:b + 1] != want).sum().item()} outputs differ"
        assert torch.equal(u8(st[b:b + 1]), u8(want_st)), f"{what} sequence {b} ({k.shape[2]} keys): row_stats differ"
    assert torch.isfinite(out).all()
    return out, st


# ---- 1. bits per sequence --------------------------------------------------------------------------------------------------------
CASES1 = [(name, dt, s, causal) for name, dts in (("A", DTYPES), ("B", DTYPES[:1]), ("C", DTYPES[:1])) for dt in dts for s in (1, 3, 8)
          for causal in (False, True) if not causal or s <= min(SETS[name][0])]


@pytest.mark.parametrize("name, dtype, s, causal", CASES1, ids=[f"{n}-{DT_ID[dt]}-s{s}-{'causal' if c else 'full'}" for n, dt, s, c in CASES1])
def test_bits_per_sequence(name, dtype, s, causal):
    cache, seqs = _paged(name, dtype)
    _check_bits(cache, seqs, _raw(name, dtype), _q(name, dtype, len(seqs), s), causal)


def test_bits_per_sequence_bshd():
    cache, seqs = _paged("B", torch.float16)
    out, _ = _check_bits(cache, seqs, _raw("B", torch.float16), _q("B", torch.float16, len(seqs), 3), True, layout="bshd")
    assert out.shape == (len(seqs), 3, SETS["B"][2], SETS["B"][1])


# ---- 2. independence of the batch and of max_len -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name, wide", [("A", 40), ("B", 200)])
def test_rows_do_not_depend_on_the_batch_or_on_max_len(name, wide):
    """`wide` pages per sequence: 640 resp. 3200 keys of max_len - other workspace strides, a grid of 16 resp. 25 chunks."""
    from lqer_amd import attention_flexible_paged

    dt = torch.float16
    cache, seqs = _paged(name, dt)
    q = _q(name, dt, len(seqs), 3)
    sc = q.shape[3] ** -0.5
    out, st = attention_flexible_paged(q, cache, seqs, sc, causal=False, return_stats=True)
    pick = [2, 0]
    sub, sub_st = attention_flexible_paged(q[pick], cache, [seqs[i] for i in pick], sc, causal=False, return_stats=True)
    assert torch.equal(u8(sub), u8(out[pick])) and torch.equal(u8(sub_st), u8(st[pick]))
    big, big_seqs = _build(name, dt, max_pages_per_seq=wide, spare=3)
    assert big.pt.max_len == 16 * wide > cache.pt.max_len
    wout, wst = attention_flexible_paged(q, big, big_seqs, sc, causal=False, return_stats=True)
    assert torch.equal(u8(wout), u8(out)) and torch.equal(u8(wst), u8(st))


# ---- 3. pages anywhere, dirty ------------------------------------------------------------------------------------------------------
def _pool_spans(cache, pages, slot):
    """Byte spans [lo, hi) of the pool that belong to `pages` (all kv heads, the four sections) and to `slot`'s staging rows - from the
    header's layout."""
    up = lambda v: (v + 255) // 256 * 256
    hk, d, esz = cache.kv_heads, cache.head_dim, torch.empty((), dtype=cache.dtype).element_size()
    items = cache.num_pages * hk
    spans, at = [], 0
    for per_item in (16 * d, d, 16 * d, d):
        spans += [(at + p * hk * per_item, at + (p + 1) * hk * per_item) for p in pages]
        at += up(items * per_item)
    per_slot = hk * 16 * d * esz
    spans.append((at + slot * per_slot, at + (slot + 1) * per_slot))
    assert at + up(cache.max_seqs * per_slot) == cache.buf.numel()
    return spans


def _same_live_bytes(dense, ref, t, what):
    """The sections' live part of two dense caches of one capacity: K codes and K exponents of every block up to the length (an append
    rewrites a touched block whole, zero-padded), V codes and V exponents of the keys below the length (a V row is written once, when
    its key arrives: the rest of an open block is whatever the buffer held, on both sides), staging rows 0 .. t % 16 - 1."""
    from lqer_amd.kvcache import _sections

    assert dense.capacity == ref.capacity and dense.length == ref.length == t
    hk, d = dense.kv_heads, dense.head_dim
    esz = torch.empty((), dtype=dense.dtype).element_size()
    secs, total = _sections(dense.dtype, 1, hk, dense.capacity, d)
    assert total == dense.buf.numel() == ref.buf.numel()
    blocks, full = pages_of(t), t // 16
    for name, at, per_block in secs:
        row = 16 * d * esz if per_block is None else (dense.capacity // 16) * per_block
        live = torch.zeros(row, dtype=torch.bool, device=DEV)
        if name == "k_stage":
            live[:(t % 16) * d * esz] = True
        elif name in ("k_codes", "k_exps"):
            live[:blocks * per_block] = True
        elif name == "v_codes":
            live[:t * d] = True
        else:  # v_exps: [block][d / 16][16 keys]
            live[:full * per_block] = True
            if t % 16:
                live[full * per_block:blocks * per_block].view(d // 16, 16)[:, :t % 16] = True
        assert int(live.sum()) > 0 or name == "k_stage"
        a, r = (x.buf[at:at + hk * row].view(hk, row)[:, live] for x in (dense, ref))
        assert torch.equal(a, r), f"{what}: section {name} differs in {(a != r).sum().item()} of {a.numel()} live bytes"


@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
def test_pages_anywhere_and_dirty(dtype):
    from lqer_amd import PagedKVCache

    d, h, hk = 48, 4, 2
    raw = lambda n, seed: tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dtype, seed, 2.0))
    lens0 = (37, 37, 40)
    first = [raw(n, 2000 + i) for i, n in enumerate(lens0)]
    cache = PagedKVCache(sum(map(pages_of, lens0)) + pages_of(21) + pages_of(33), 5, hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=3)
    seqs = [cache.alloc() for _ in lens0]
    for t in range(max(lens0)):  # interleaved single-token appends: the sequences' pages interleave
        live = [i for i, n in enumerate(lens0) if t < n]
        cache.append([seqs[i] for i in live], torch.cat([first[i][0][:, :, t:t + 1] for i in live]), torch.cat([first[i][1][:, :, t:t + 1] for i in live]))
    rows = [cache.pt.table[cache.pt.slot(s)][:3] for s in seqs]
    assert rows[0][0] < rows[1][0] < rows[2][0] < rows[0][1]  # interleaved indeed
    # free the middle one and dirty everything it owned
    mid_slot, mid_pages = cache.pt.slot(seqs[1]), rows[1]
    cache.free(seqs[1])
    for lo, hi in _pool_spans(cache, mid_pages, mid_slot):
        cache.buf[lo:hi].fill_(0xFF)
    # a new sequence on those pages and that slot; two more on fresh pages
    patterns = {"5, 27, singles": (35, [5, 27, 1, 1, 1]), "16, singles": (21, [16] + [1] * 5), "one call": (33, [33])}
    new, new_raw, new_pat = [], [], []
    for i, (pname, (n, pattern)) in enumerate(patterns.items()):
        s, (k, v) = cache.alloc(), raw(n, 2100 + i)
        at = 0
        for step in pattern:
            cache.append([s], k[:, :, at:at + step], v[:, :, at:at + step])
            at += step
        new.append(s), new_raw.append((k, v)), new_pat.append(pattern)
    assert cache.pt.slot(new[0]) == mid_slot and sorted(cache.pt.table[mid_slot][:3]) == sorted(mid_pages) and cache.pages_free == 0
    live_seqs, live_raw = [seqs[0], seqs[2]] + new, [first[0], first[2]] + new_raw
    live_pat = [[1] * 37, [1] * 40] + new_pat
    for s_rows, causal in ((1, False), (3, True), (8, False)):
        _check_bits(cache, live_seqs, live_raw, F._randn((len(live_seqs), h, s_rows, d), dtype, 31 + s_rows, 3.0).to(DEV), causal, what="dirty pool:")
    for s, (k, v), pattern in zip(live_seqs, live_raw, live_pat):
        dense = cache.to_dense(s)
        _same_live_bytes(dense, KV._cache(k, v, pattern, capacity=dense.capacity), k.shape[2], f"sequence {s} appended as {pattern[:3]}..")


# ---- 4. isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length, n", [(21, 1), (15, 1), (16, 1), (30, 5)])  # inside a page; filling one; opening one; across a boundary
def test_append_and_attention_stay_inside_their_pages(length, n):
    from lqer_amd import PagedKVCache, attention_flexible_paged
    from lqer_amd import _lib

    dt, d, h, hk, stride = torch.float16, 48, 4, 2, 4
    cache = PagedKVCache(9, 3, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=1, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(3, stride)  # (random bytes: a dirty pool, a dirty table)
    seqs = [cache.alloc() for _ in range(3)]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t, d), dt, 3000 + i, 2.0)) for i, t in enumerate((40, length + n, 18))]
    for s, (k, v), t in zip(seqs, raws, (40, length, 18)):
        cache.append([s], k[:, :, :t], v[:, :, :t])
    torch.cuda.synchronize()
    snap = g_pool.payload.clone()
    k, v = raws[1]
    cache.append([seqs[1]], k[:, :, length:], v[:, :, length:])
    torch.cuda.synchronize()
    g_pool.check(), g_tbl.check()
    slot = cache.pt.slot(seqs[1])
    touched = [cache.pt.table[slot][i] for i in range(length // 16, (length + n - 1) // 16 + 1)]
    allowed = torch.zeros(snap.numel(), dtype=torch.bool, device=DEV)
    for lo, hi in _pool_spans(cache, touched, slot):
        allowed[lo:hi] = True
    changed = g_pool.payload != snap
    assert not bool((changed & ~allowed).any()), f"{int((changed & ~allowed).sum())} bytes changed outside pages {touched} and slot {slot}'s staging rows"
    assert bool(changed.any())
    # the attention only reads the pool, and stays inside its workspace
    q = F._randn((3, h, 2, d), dt, 77, 3.0).to(DEV)
    g_ws = _guard.guarded(_lib.lib().lqer_attention_q_decode_paged_workspace_bytes(3, h, hk, 2, cache.pt.max_len, d), align=16, fill=0xFF, name="workspace")
    before = g_pool.payload.clone()
    out, st = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True, ws=g_ws.payload)
    torch.cuda.synchronize()
    g_ws.check(), g_pool.check(), g_tbl.check()
    assert torch.equal(g_pool.payload, before)
    for b, (kb, vb) in enumerate(raws):
        want, want_st = _want(q[b:b + 1], kb, vb, True)
        assert torch.equal(u8(out[b:b + 1]), u8(want)) and torch.equal(u8(st[b:b + 1]), u8(want_st))


# ---- 5. more than 8 query rows: gather, then the prefill kernel over the dense cache --------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_more_than_eight_query_rows_through_to_dense(causal):
    from lqer_amd import attention_flexible, attention_flexible_cached, attention_flexible_paged

    dt = torch.float16
    cache, seqs = _paged("A", dt)
    (k, v), seq = _raw("A", dt)[4], seqs[4]  # 37 keys
    q = _q("A", dt, 1, 20)
    with pytest.raises(ValueError):
        attention_flexible_paged(q, cache, [seq], 48 ** -0.5)
    dense = cache.to_dense(seq)
    assert dense.length == 37 and dense.batch == 1
    got, got_st = attention_flexible_cached(q, dense, 48 ** -0.5, causal=causal, kernel="prefill", return_stats=True)
    want, want_st = attention_flexible(q, k, v, CFG, CFG, 48 ** -0.5, causal=causal, kernel="prefill", return_stats=True)
    assert torch.equal(u8(got), u8(want)) and torch.equal(u8(got_st), u8(want_st))


# ---- 6. the stored values against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
def test_dequantized_equals_the_oracle(dtype):
    cache, seqs = _paged("A", dtype)
    for s, (k, v) in zip(seqs, _raw("A", dtype)):
        want_k, want_v = KV._oracle(k.cpu(), v.cpu())
        got_k, got_v = (x.cpu() for x in cache.dequantized(s))
        assert got_k.shape == k.shape and got_k.dtype == torch.float32
        assert torch.equal(got_k, want_k), f"{k.shape[2]} keys, K: {(got_k != want_k).sum().item()} of {want_k.numel()} differ"
        assert torch.equal(got_v, want_v), f"{k.shape[2]} keys, V: {(got_v != want_v).sum().item()} of {want_v.numel()} differ"


# ---- what the Python side refuses (nothing is launched) ------------------------------------------------------------------------------
def test_python_refusals_leave_the_pool_untouched():
    from lqer_amd import PagedKVCache, attention_flexible_paged

    dt, d, hk = torch.float16, 48, 2
    cache = PagedKVCache(3, 3, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=2)
    a, b, c = (cache.alloc() for _ in range(3))
    k, v = (x.to(DEV) for x in KV._kv((2, hk, 20, d), dt, 4000))
    cache.append([a], k[:1], v[:1])
    snap, state = cache.buf.clone(), (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:])
    for seqs, kk in [([b, c], k), ([a], k[:1, :, :13]), ([b, b], k), ([b, 9], k)]:  # out of pages; beyond max_pages_per_seq; twice; unknown
        with pytest.raises((RuntimeError, ValueError, KeyError)):
            cache.append(seqs, kk, kk)
    cache.free(c)
    with pytest.raises(KeyError):
        cache.append([c], k[:1], v[:1])
    torch.cuda.synchronize()
    assert torch.equal(cache.buf, snap) and state == (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:])
    q = F._randn((1, 4, 2, d), dt, 5).to(DEV)
    for what, qq, seqs in [("an empty sequence", q, [b]), ("s > 8", F._randn((1, 4, 9, d), dt, 5).to(DEV), [a]), ("dtype", q.float(), [a]),
                           ("device", q.cpu(), [a]), ("head count", q[:, :3], [a]), ("head dim", q[..., :32], [a]), ("batch", q, [a, b]),
                           ("named twice", q.repeat(2, 1, 1, 1), [a, a]), ("freed", q, [c])]:
        with pytest.raises(ValueError):
            attention_flexible_paged(qq, cache, seqs, 1.0)
            pytest.fail(what)
    short = cache.alloc()
    cache.append([short], k[:1, :, :5], v[:1, :, :5])
    with pytest.raises(ValueError):  # causal with more query rows than keys
        attention_flexible_paged(F._randn((1, 4, 8, d), dt, 6).to(DEV), cache, [short], 1.0, causal=True)
    torch.cuda.synchronize()

"""Per-sequence token counts on the paged KV pool, on the GPU (lqer_kv_pool_append_ragged / lqer_attention_q_paged_ragged;
csrc/kv_cache.hip's and csrc/attn_q.hip's ragged instantiations; PagedKVCache.append_ragged, attention_flexible_paged_ragged).

The contract is an equality of bits per sequence.  After one append over sequences with counts of their own the pool holds, for
every sequence, the bytes that a uniform append of that sequence alone leaves; the rows of a sequence in out and row_stats of one
attention call over such a batch are those of the kernel on the raw K and V of that sequence alone (attention_flexible with batch 1 -
never the paged code itself).  Every comparison is torch.equal on the bytes; there is no tolerance in this file.  The length sets are
test_gpu_kv_paged.py's; the counts cross the 8 rows of the decode kernel (8, 9), the 32-query wave (33) and the 128-query workgroup
(129, 200), and include 0 and 1."""
import ctypes as C
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
from test_gpu_kv_paged import SETS, _paged, _pool_spans, _q, _raw, _same_live_bytes, u8

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES = F.CFG, F.DEV, F.DTYPES
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
F16 = torch.float16
pages_of = lambda n: (n + 15) // 16
starts_of = lambda counts: [sum(counts[:b]) for b in range(len(counts) + 1)]


def _packed(xs, los, counts):
    """Rows los[i] .. los[i] + counts[i] - 1 of every xs[i] [1, heads, L, d], packed as [sum(counts), heads, d]."""
    return torch.cat([x[0, :, lo:lo + c].transpose(0, 1) for x, lo, c in zip(xs, los, counts)]).contiguous()


# ---- 1. append bits ----------------------------------------------------------------------------------------------------------------
ROUNDS = {"A": ((1, 7, 16, 0, 20), (0, 8, 0, 17, 17)), "B": ((255, 15, 31, 47), (0, 241, 226, 253)), "C": ((2047, 1, 5), (1, 2048, 0))}
CASES1 = [("A", dt) for dt in DTYPES] + [("B", F16), ("C", F16)]


@pytest.mark.parametrize("name, dtype", CASES1, ids=[f"{n}-{DT_ID[dt]}" for n, dt in CASES1])
def test_append_bits(name, dtype):
    """Two ragged rounds - a count of 0 on an empty and on a non-empty sequence, a block left open, one closed exactly, two touched from
    empty, appends that start at len % 16 = 15, a 2048-key prompt beside one-key steps in one launch - against a pool built by one
    uniform append per sequence and round; then one more key, uniformly, on both: the staging rows were left right."""
    from lqer_amd import PagedKVCache

    lens, d, _, hk = SETS[name]
    r1, r2 = ROUNDS[name]
    assert tuple(a + b for a, b in zip(r1, r2)) == lens
    raws = _raw(name, dtype)
    pages = sum(pages_of(n + 1) for n in lens)
    rag, ref = (PagedKVCache(pages, len(lens), hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=max(pages_of(n + 1) for n in lens)) for _ in range(2))
    seqs = [rag.alloc() for _ in lens]
    assert seqs == [ref.alloc() for _ in lens]
    at = [0] * len(lens)
    for counts in (r1, r2):
        free = rag.pages_free
        rag.append_ragged(seqs, _packed([r[0] for r in raws], at, counts), _packed([r[1] for r in raws], at, counts), counts)
        for s, (k, v), lo, c in zip(seqs, raws, at, counts):
            if c:
                ref.append([s], k[:, :, lo:lo + c], v[:, :, lo:lo + c])
        at = [lo + c for lo, c in zip(at, counts)]
        assert [rag.length(s) for s in seqs] == at == [ref.length(s) for s in seqs]
        assert rag.pages_free == ref.pages_free == free - sum(pages_of(t) - pages_of(t - c) for t, c in zip(at, counts))

    def same(what):
        for i, s in enumerate(seqs):
            t = rag.length(s)
            if t == 0:
                continue
            _same_live_bytes(rag.to_dense(s), ref.to_dense(s), t, f"{what}: sequence {i} ({t} keys)")
            for got, want in zip(rag.dequantized(s), ref.dequantized(s)):
                assert torch.equal(got, want), (what, i, t)

    same("after round 1 and 2")
    k1, v1 = (x.to(DEV) for x in KV._kv((len(lens), hk, 1, d), dtype, 6000 + ord(name), 2.0))
    rag.append(seqs, k1, v1), ref.append(seqs, k1, v1)
    same("after one more key")


# ---- 2. / 3. attention bits ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(name, dtype, i, c, causal, kernel):
    """The comparator for sequence i of a set with c query rows - the queries _q(name, dtype, n, c)[i] -: attention_flexible on the raw
    K and V of that sequence alone, as rows [c, h, d] and [c, h, 2].  Made once, never written."""
    from lqer_amd import attention_flexible

    k, v = _raw(name, dtype)[i]
    q1 = _q(name, dtype, len(SETS[name][0]), c)[i:i + 1]
    out, st = attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, causal=causal, kernel=kernel, return_stats=True)
    return out[0].transpose(0, 1).contiguous(), st[0].transpose(0, 1).contiguous()


def _queries(name, dtype, counts, pick=None):
    n = len(SETS[name][0])
    pick = range(n) if pick is None else pick
    return torch.cat([_q(name, dtype, n, c)[i].transpose(0, 1) for i, c in zip(pick, counts) if c]).contiguous()


def _check_rows(name, dtype, counts, causal, out, st, kernel, pick=None, what=""):
    """Every sequence's rows of a packed out / stats against its comparator: the decode kernel's up to 8 rows under "auto"."""
    pick = list(range(len(SETS[name][0]))) if pick is None else list(pick)
    at = starts_of(counts)
    for b, (i, c) in enumerate(zip(pick, counts)):
        if not c:
            continue
        want, want_st = _want(name, dtype, i, c, causal, "decode" if kernel == "auto" and c <= 8 else "prefill")
        got, got_st = out[at[b]:at[b + 1]], st[at[b]:at[b + 1]]
        assert got.shape == want.shape and got_st.shape == want_st.shape
        assert torch.equal(u8(got), u8(want)), f"{what} sequence {i} ({SETS[name][0][i]} keys, {c} rows): {(got != want).sum().item()} outputs differ"
        assert torch.equal(u8(got_st), u8(want_st)), f"{what} sequence {i} ({SETS[name][0][i]} keys, {c} rows): row_stats differ"


CASES2 = ([("A", dt, False, (9, 1, 33, 3, 20)) for dt in DTYPES] + [("A", dt, True, (1, 8, 16, 9, 33)) for dt in DTYPES] +
          [("B", F16, False, (200, 1, 129, 33)), ("B", F16, True, (200, 1, 129, 33)), ("C", F16, True, (33, 1, 5))])


@pytest.mark.parametrize("kernel", ["prefill", "auto"])
@pytest.mark.parametrize("name, dtype, causal, counts", CASES2, ids=[f"{n}-{DT_ID[dt]}-{'causal' if c else 'full'}" for n, dt, c, _ in CASES2])
def test_attention_bits(name, dtype, causal, counts, kernel):
    from lqer_amd import attention_flexible_paged_ragged

    cache, seqs = _paged(name, dtype)
    q = _queries(name, dtype, counts)
    out, st = attention_flexible_paged_ragged(q, cache, seqs, counts, q.shape[2] ** -0.5, causal=causal, return_stats=True, kernel=kernel)
    assert out.shape == q.shape and out.dtype == q.dtype and st.shape == (*q.shape[:2], 2) and st.dtype == torch.float32
    _check_rows(name, dtype, counts, causal, out, st, kernel)
    assert torch.isfinite(out).all()
    alone = attention_flexible_paged_ragged(q, cache, seqs, counts, q.shape[2] ** -0.5, causal=causal, kernel=kernel)  # (without the statistics)
    assert torch.equal(u8(alone), u8(out))


def test_auto_is_what_attention_flexible_paged_gives_each_sequence_alone():
    from lqer_amd import attention_flexible_paged, attention_flexible_paged_ragged

    name = "B"
    cache, seqs = _paged(name, F16)
    # every call's rows one range of q; a decode group split by a chunk (its rows gathered); the chunks split by a decoder
    for counts in ((200, 1, 8, 33), (1, 200, 1, 33), (33, 1, 129, 1)):
        q = _queries(name, F16, counts)
        out, st = attention_flexible_paged_ragged(q, cache, seqs, counts, 0.125, causal=True, return_stats=True)
        at = starts_of(counts)
        for b, c in enumerate(counts):
            q1 = q[at[b]:at[b + 1]].transpose(0, 1).unsqueeze(0)
            want, want_st = attention_flexible_paged(q1, cache, [seqs[b]], 0.125, causal=True, return_stats=True, kernel="auto")
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want[0].transpose(0, 1))), (counts, b)
            assert torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st[0].transpose(0, 1))), (counts, b)


# ---- the C call itself: a bound max_s, a q buffer and an out buffer of the caller's ---------------------------------------------------
def _c_ragged(cache, seqs, counts, q, out, st, causal, max_s=None, max_len=None, total=None, ws=None):
    """lqer_attention_q_paged_ragged as it stands: every sequence of the call is handed over, a count of 0 included; q / out [rows, h, d]
    views with any token and head stride."""
    from lqer_amd import _lib, ops
    from lqer_amd.kvcache import _pair

    L, f = _lib.lib(), cache.fmts
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[s] for s in slots]
    h, d = q.shape[1], q.shape[2]
    max_s = max(counts) if max_s is None else max_s
    max_len = min((max(lens) + 127) // 128 * 128, cache.pt.max_len) if max_len is None else max_len
    if ws is None:
        ws = torch.full((L.lqer_attention_q_paged_ragged_workspace_bytes(len(seqs), h, cache.kv_heads, max_s, max_len, d),), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(q.device):
        _lib.check(L.lqer_attention_q_paged_ragged(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(),
                                                   st.data_ptr() if st is not None else None, ops.dtype_code(q), len(seqs), h, cache.kv_heads,
                                                   cache._call_starts(counts), max_s, sum(counts) if total is None else total, d, _pair(q),
                                                   _pair(out), d ** -0.5, int(causal), C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), C.byref(f[3]),
                                                   ws.data_ptr(), ws.numel(), ops._stream(q.device)), "lqer_attention_q_paged_ragged")


def _padded(rows, h, d, dtype, spare, pad, fill):
    """A [rows, h, d] view with `spare` tokens behind it and a token stride padded by `pad` elements, over a buffer of `fill` bytes."""
    base = torch.full(((rows + spare) * (h * d + pad) * torch.empty((), dtype=dtype).element_size(),), fill, dtype=torch.uint8, device=DEV).view(dtype)
    return base, base.as_strided((rows, h, d), (h * d + pad, d, 1))


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_the_bounds_or_the_buffers():
    """Sequences 0 (255 keys, 200 rows) and 2 (257 keys, 129 rows) of set B: alone, inside the batch and inside the reversed batch; with
    max_s tight and at 4096; from a q buffer with spare tokens behind `total` and a padded token stride (and `total` beyond the rows in
    use); on the tight pool and on one with 200 pages per sequence (other image strides, other grids)."""
    from lqer_amd import attention_flexible_paged_ragged
    from test_gpu_kv_paged import _build

    name, counts = "B", (200, 1, 129, 33)
    n, (_, d, h, _) = len(counts), SETS[name]
    tight, wide = _paged(name, F16), _build(name, F16, max_pages_per_seq=200, spare=3)
    assert wide[0].pt.max_len == 3200 and tight[0].pt.max_len == 304
    for i in (0, 2):
        want, want_st = (u8(x) for x in _want(name, F16, i, counts[i], True, "prefill"))
        for cache, seqs in (tight, wide):
            for order in ([i], list(range(n)), list(range(n))[::-1]):
                cs = [counts[j] for j in order]
                at, b = starts_of(cs), order.index(i)
                q = _queries(name, F16, cs, order)
                out, st = attention_flexible_paged_ragged(q, cache, [seqs[j] for j in order], cs, d ** -0.5, causal=True, return_stats=True, kernel="prefill")
                assert torch.equal(u8(out[at[b]:at[b + 1]]), want) and torch.equal(u8(st[at[b]:at[b + 1]]), want_st), (i, order, cache.pt.max_len)
                for max_s, max_len in ((max(cs), None), (4096, None), (4096, cache.pt.max_len)):
                    total = sum(cs)
                    _, qv = _padded(total, h, d, F16, 5, 24, 0xFF)
                    qv.copy_(q)
                    obase, ov = _padded(total, h, d, F16, 5, 8, 0x5A)
                    sv = torch.full((total + 5, h, 2), 7.0, dtype=torch.float32, device=DEV)
                    _c_ragged(cache, [seqs[j] for j in order], cs, qv, ov, sv, True, max_s=max_s, max_len=max_len, total=total + 5)
                    assert torch.equal(u8(ov[at[b]:at[b + 1]]), want) and torch.equal(u8(sv[at[b]:at[b + 1]]), want_st), (i, order, max_s, max_len)
                    assert torch.equal(u8(ov), u8(out)) and bool((sv[total:] == 7.0).all())
                    keep = torch.ones_like(obase, dtype=torch.bool)
                    keep.as_strided(ov.shape, ov.stride()).fill_(False)
                    assert bool((u8(obase[keep]) == 0x5A).all())  # the spare tokens and the padding of out keep their bytes


# ---- 5. zero counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["prefill", "auto"])
def test_zero_counts(kernel):
    from lqer_amd import attention_flexible_paged_ragged

    name, counts = "A", (0, 8, 0, 9, 33)
    _, d, h, _ = SETS[name]
    cache, seqs = _paged(name, F16)
    q = _queries(name, F16, counts)
    out, st = attention_flexible_paged_ragged(q, cache, seqs, counts, d ** -0.5, causal=True, return_stats=True, kernel=kernel)
    assert out.shape == (50, h, d)
    _check_rows(name, F16, counts, True, out, st, kernel)
    # the other sequences' rows are what they are without the two: the call over sequences 1, 3, 4 alone
    sub, sub_st = attention_flexible_paged_ragged(q, cache, [seqs[i] for i in (1, 3, 4)], (8, 9, 33), d ** -0.5, causal=True, return_stats=True, kernel=kernel)
    assert torch.equal(u8(sub), u8(out)) and torch.equal(u8(sub_st), u8(st))
    none = attention_flexible_paged_ragged(q[:0], cache, seqs, (0,) * 5, d ** -0.5, causal=True, kernel=kernel)
    assert none.shape == (0, h, d)


def test_zero_counts_in_the_c_call_write_nothing():
    """All five sequences handed to the library, two with S_b = 0: their workgroups leave at once, the others' rows are the
    comparator's, and an out filled with a pattern keeps it everywhere else."""
    name, counts = "A", (0, 8, 0, 9, 33)
    _, d, h, _ = SETS[name]
    cache, seqs = _paged(name, F16)
    total = sum(counts)
    q = _queries(name, F16, counts)
    obase, ov = _padded(total, h, d, F16, 3, 16, 0x5A)
    sv = torch.full((total + 3, h, 2), 7.0, dtype=torch.float32, device=DEV)
    _c_ragged(cache, seqs, counts, q, ov, sv, True, total=total + 3)
    _check_rows(name, F16, counts, True, ov, sv[:total], "prefill")
    keep = torch.ones_like(obase, dtype=torch.bool)
    keep.as_strided(ov.shape, ov.stride()).fill_(False)
    assert bool((u8(obase[keep]) == 0x5A).all()) and bool((sv[total:] == 7.0).all())
    # every count 0: nothing at all is written
    obase.view(torch.uint8).fill_(0x5A)
    _c_ragged(cache, seqs, (0,) * 5, q, ov, sv, True, max_s=1, total=total)
    torch.cuda.synchronize()
    assert bool((u8(obase) == 0x5A).all())


# ---- 6. footprint ------------------------------------------------------------------------------------------------------------------
def test_footprint():
    """Pool and workspace start at 0xFF; k / v / q are guarded inputs; out, statistics, workspace, pool and table carry guard zones; an
    append writes only the pages and staging rows of the sequences it gives keys to, the attention writes nothing of the pool."""
    from lqer_amd import PagedKVCache, _lib

    dt, d, h, hk, stride = F16, 48, 4, 2, 4
    cache = PagedKVCache(11, 4, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=0xFF, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(4, stride)
    seqs = [cache.alloc() for _ in range(4)]
    have, counts = (40, 15, 18, 0), (1, 20, 0, 33)  # inside a page; from len % 16 = 15 across two boundaries; nothing; a prompt from empty
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t + c, d), dt, 3300 + i, 2.0)) for i, (t, c) in enumerate(zip(have, counts))]
    for s, (k, v), t in zip(seqs, raws, have):
        if t:
            cache.append([s], k[:, :, :t], v[:, :, :t])
    total = sum(counts)
    g_k, g_v = (_guard.guarded(total * hk * d * 2, align=16, name=nm).load(_packed([r[j] for r in raws], have, counts)) for j, nm in ((0, "k_new"), (1, "v_new")))
    torch.cuda.synchronize()
    snap = g_pool.payload.clone()
    cache.append_ragged(seqs, g_k.view(dt).view(total, hk, d), g_v.view(dt).view(total, hk, d), counts)
    torch.cuda.synchronize()
    g_pool.check(), g_tbl.check(), g_k.unchanged(), g_v.unchanged()
    allowed = torch.zeros(snap.numel(), dtype=torch.bool, device=DEV)
    for s, t, c in zip(seqs, have, counts):
        if c:
            slot = cache.pt.slot(s)
            for lo, hi in _pool_spans(cache, [cache.pt.table[slot][i] for i in range(t // 16, (t + c - 1) // 16 + 1)], slot):
                allowed[lo:hi] = True
    changed = g_pool.payload != snap
    assert bool(changed.any()) and not bool((changed & ~allowed).any()), f"{int((changed & ~allowed).sum())} bytes changed outside the pages and staging rows of the sequences given keys"
    # the attention: every sequence handed to the library, the one without new keys with a count of 0
    q_counts = (1, 20, 0, 33)
    lens = [t + c for t, c in zip(have, counts)]
    qs = [F._randn((1, h, c, d), dt, 80 + i, 3.0).to(DEV) for i, c in enumerate(q_counts)]
    g_q = _guard.guarded(total * h * d * 2, align=16, name="q").load(_packed(qs, [0] * 4, q_counts))
    max_len = 64
    need = _lib.lib().lqer_attention_q_paged_ragged_workspace_bytes(4, h, hk, max(q_counts), max_len, d)
    g_ws = _guard.guarded(need, align=16, fill=0xFF, name="workspace")
    g_out = _guard.guarded(total * h * d * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(total * h * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(total, h, d), g_st.view(torch.float32).view(total, h, 2)
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    _c_ragged(cache, seqs, q_counts, g_q.view(dt).view(total, h, d), out, st, True, max_len=max_len, ws=g_ws.payload)
    torch.cuda.synchronize()
    g_ws.check(), g_out.check(), g_st.check(), g_pool.check(), g_tbl.check(), g_q.unchanged()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)
    from lqer_amd import attention_flexible

    at = starts_of(q_counts)
    for b, ((k, v), c) in enumerate(zip(raws, q_counts)):
        if c:
            want, want_st = attention_flexible(qs[b], k[:, :, :lens[b]], v[:, :, :lens[b]], CFG, CFG, d ** -0.5, causal=True, kernel="prefill", return_stats=True)
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want[0].transpose(0, 1))) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st[0].transpose(0, 1))), b
    assert torch.isfinite(out).all()


# ---- 7. one mixed step end to end ----------------------------------------------------------------------------------------------------
def test_one_mixed_step_end_to_end():
    """Six decoders and two prompt chunks (33 rows on 40 keys, 129 rows from empty) in one append_ragged and one
    attention_flexible_paged_ragged(causal=True), against the step done per distinct count on a second pool."""
    from lqer_amd import PagedKVCache, attention_flexible_paged, attention_flexible_paged_ragged

    dt, d, h, hk = F16, 64, 8, 2
    have, counts = (254, 255, 256, 299, 15, 2047, 40, 0), (1, 1, 1, 1, 1, 1, 33, 129)
    lens = [t + c for t, c in zip(have, counts)]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t, d), dt, 3400 + i, 2.0)) for i, t in enumerate(lens)]
    rag, ref = (PagedKVCache(sum(map(pages_of, lens)), 8, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=max(map(pages_of, lens))) for _ in range(2))
    seqs = [rag.alloc() for _ in lens]
    assert seqs == [ref.alloc() for _ in lens]
    for cache in (rag, ref):
        for s, (k, v), t in zip(seqs, raws, have):
            if t:
                cache.append([s], k[:, :, :t], v[:, :, :t])
    new = lambda j, idx: torch.cat([raws[i][j][:, :, have[i]:] for i in idx])
    rag.append_ragged(seqs, _packed([r[0] for r in raws], have, counts), _packed([r[1] for r in raws], have, counts), counts)
    ref.append(seqs[:6], new(0, range(6)), new(1, range(6)))
    ref.append(seqs[6:7], new(0, [6]), new(1, [6])), ref.append(seqs[7:], new(0, [7]), new(1, [7]))
    assert [rag.length(s) for s in seqs] == lens == [ref.length(s) for s in seqs] and rag.pages_free == ref.pages_free == 0
    for i, s in enumerate(seqs):
        _same_live_bytes(rag.to_dense(s), ref.to_dense(s), lens[i], f"sequence {i}")
    qs = [F._randn((1, h, c, d), dt, 120 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    q = _packed(qs, [0] * 8, counts)
    out, st = attention_flexible_paged_ragged(q, rag, seqs, counts, d ** -0.5, causal=True, return_stats=True)
    want = [attention_flexible_paged(torch.cat(qs[:6]), ref, seqs[:6], d ** -0.5, causal=True, return_stats=True, kernel="auto")]
    want += [attention_flexible_paged(qs[i], ref, [seqs[i]], d ** -0.5, causal=True, return_stats=True, kernel="auto") for i in (6, 7)]
    want_out = torch.cat([w[0].transpose(1, 2).reshape(-1, h, d) for w in want])
    want_st = torch.cat([w[1].transpose(1, 2).reshape(-1, h, 2) for w in want])
    assert torch.equal(u8(out), u8(want_out)) and torch.equal(u8(st), u8(want_st)) and torch.isfinite(out).all()
    # ... and against the kernels on the raw tensors: the decode kernel for the one-row sequences, the prefill kernel for the chunks
    from lqer_amd import attention_flexible

    at = starts_of(counts)
    for i, ((k, v), c) in enumerate(zip(raws, counts)):
        w, w_st = attention_flexible(qs[i], k, v, CFG, CFG, d ** -0.5, causal=True, kernel="decode" if c <= 8 else "prefill", return_stats=True)
        assert torch.equal(u8(out[at[i]:at[i + 1]]), u8(w[0].transpose(0, 1))) and torch.equal(u8(st[at[i]:at[i + 1]]), u8(w_st[0].transpose(0, 1))), i


# ---- 8. what the Python side refuses (nothing is launched) ---------------------------------------------------------------------------
def test_python_refusals_leave_the_pool_untouched():
    from lqer_amd import PagedKVCache, attention_flexible_paged_ragged

    dt, d, hk, h = F16, 48, 2, 4
    cache = PagedKVCache(4, 4, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=2)
    a, b, c, short = (cache.alloc() for _ in range(4))
    k, v = (x.to(DEV) for x in KV._kv((1, hk, 30, d), dt, 4200))
    cache.append([a], k, v)
    cache.append([short], k[:, :, :5], v[:, :, :5])
    cache.free(c)
    torch.cuda.synchronize()
    books = lambda: (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:], cache.pt.pages_of[:])
    snap, state = cache.buf.clone(), books()
    q = F._randn((21, h, d), dt, 5).to(DEV)
    for what, qq, seqs, counts, kw in [("len(counts) != len(seqs)", q, [a, short], [21], {}),
                                       ("a negative count", q, [a, short], [22, -1], {}),
                                       ("sum(counts) != q.shape[0]", q, [a, short], [20, 2], {}),
                                       ("causal with counts[b] > length_b", q, [a, short], [15, 6], dict(causal=True)),
                                       ("an empty sequence with a count", q, [a, b], [20, 1], {}),
                                       ("freed", q, [a, c], [20, 1], {}), ("named twice", q, [a, a], [20, 1], {}),
                                       ("dtype", q.float(), [a, short], [20, 1], {}), ("device", q.cpu(), [a, short], [20, 1], {}),
                                       ("head count", q[:, :3], [a, short], [20, 1], {}), ("head dim", q[..., :32], [a, short], [20, 1], {}),
                                       ("q is not [total, h, d]", q.unsqueeze(0), [a, short], [20, 1], {}),
                                       ("unknown kernel", q, [a, short], [20, 1], dict(kernel="flash")),
                                       ("a window without causal", q, [a, short], [20, 1], dict(window=64)),
                                       ("the prefill kernel beyond the window", q, [a, short], [20, 1], dict(causal=True, window=16))]:
        for kernel in ("prefill", "auto"):
            with pytest.raises(ValueError):
                attention_flexible_paged_ragged(qq, cache, seqs, counts, 1.0, **{"kernel": kernel, **kw})
                pytest.fail(what)
    kk, vv = (x[0].transpose(0, 1).contiguous() for x in (k, v))  # [30, hk, d]
    for what, seqs, kn, counts, exc in [("len(counts) != len(seqs)", [b], kk[:3], [1, 2], ValueError),
                                        ("a negative count", [b, a], kk[:3], [4, -1], ValueError),
                                        ("sum(counts) != rows", [b, a], kk[:3], [1, 1], ValueError),
                                        ("dtype", [b, a], kk[:3].float(), [1, 2], ValueError),
                                        ("head dim", [b, a], kk[:3, :, :32], [1, 2], ValueError),
                                        ("out of pages midway", [b, short], kk[:30], [17, 13], RuntimeError),
                                        ("beyond max_pages_per_seq", [b, a], kk[:4], [1, 3], RuntimeError),
                                        ("named twice", [b, b], kk[:3], [1, 2], ValueError), ("freed", [b, c], kk[:3], [1, 2], KeyError),
                                        ("unknown, beside counts of 0", [b, 99], kk[:0], [0, 0], KeyError)]:
        with pytest.raises(exc):
            cache.append_ragged(seqs, kn, kn, counts)
            pytest.fail(what)
    torch.cuda.synchronize()
    assert torch.equal(cache.buf, snap) and state == books()
    cache.append_ragged([a, b, short], kk[:0], vv[:0], [0, 0, 0])  # nothing to do: taken, and nothing happens
    torch.cuda.synchronize()
    assert torch.equal(cache.buf, snap) and state == books()
    assert attention_flexible_paged_ragged(q, cache, [a, short, b], [20, 1, 0], 1.0, causal=True).shape == q.shape  # (the same call, taken)

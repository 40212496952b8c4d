"""The prefill kernel over the paged KV pool on the GPU (lqer_attention_q_paged; csrc/kv_cache.hip's image kernels with the paged
source, csrc/attn_q.hip's per-sequence-length instantiation; attention_flexible_paged(kernel="prefill")).

The contract is an equality of bits per sequence: out[b] and row_stats[b] of ONE call over sequences of different lengths, with any
number of query rows, are those of the prefill kernel on the raw K and V of sequence b alone (attention_flexible(...,
kernel="prefill") with batch 1 - never the paged code itself).  Every comparison is torch.equal on the bytes; there is no tolerance
in this file.  The length sets are test_gpu_kv_paged.py's (A: around one page; B: around the 64-key tile and the 128-key image
padding; C: long and short in one grid); the query counts cross the 32-query wave (33) and the 128-query workgroup (129, 200)."""
import ctypes as C
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
from test_gpu_kv_paged import SETS, _build, _paged, _q, _raw, u8

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES = F.CFG, F.DEV, F.DTYPES
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
F16 = torch.float16
pages_of = lambda n: (n + 15) // 16


def _prefill(q1, k, v, causal, layout="bhsd"):
    """The comparator: the prefill kernel on the raw tensors of ONE sequence."""
    from lqer_amd import attention_flexible

    return attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, causal=causal, kernel="prefill", return_stats=True, out_layout=layout)


@functools.lru_cache(maxsize=None)
def _want(name, dtype, s, causal, i, layout="bhsd"):
    """The comparator's (out, row_stats) for sequence i of a set with the shared queries _q(name, dtype, n, s)[i]: made once, never written."""
    k, v = _raw(name, dtype)[i]
    return _prefill(_q(name, dtype, len(SETS[name][0]), s)[i:i + 1], k, v, causal, layout)


def _check_bits(name, dtype, s, causal, pick=None, layout="bhsd", cache_seqs=None, **kw):
    """One paged prefill call over sequences `pick` of the set (all of them by default), every row against the comparator."""
    from lqer_amd import attention_flexible_paged

    n = len(SETS[name][0])
    pick = list(range(n)) if pick is None else list(pick)
    cache, seqs = cache_seqs or _paged(name, dtype)
    q = _q(name, dtype, n, s)[pick]
    out, st = attention_flexible_paged(q, cache, [seqs[i] for i in pick], q.shape[3] ** -0.5, causal=causal, out_layout=layout, return_stats=True,
                                       kernel="prefill", **kw)
    assert out.dtype == q.dtype and st.shape == (*q.shape[:3], 2) and st.dtype == torch.float32
    for b, i in enumerate(pick):
        want, want_st = _want(name, dtype, s, causal, i, layout)
        keys = SETS[name][0][i]
        assert out[b:b + 1].shape == want.shape
        assert torch.equal(u8(out[b:b + 1]), u8(want)), f"sequence {i} ({keys} keys), s = {s}: {(out[b:b + 1] != want).sum().item()} outputs differ"
        assert torch.equal(u8(st[b:b + 1]), u8(want_st)), f"sequence {i} ({keys} keys), s = {s}: row_stats differ"
    assert torch.isfinite(out).all()
    return out, st


# ---- 1. bits per sequence --------------------------------------------------------------------------------------------------------
CASES1 = ([("A", dt, s, False, None) for dt in DTYPES for s in (9, 20, 33)] +          # 1, 15, 16, 17, 37 keys in one call
          [("A", dt, s, True, (2, 3, 4)) for dt in DTYPES for s in (9, 16)] +          # causal: the sequences of 16, 17 and 37 keys
          [("B", F16, s, causal, None) for s in (33, 129, 200) for causal in (False, True)] +
          [("C", F16, 33, False, None), ("C", F16, 33, True, (0, 1))])


@pytest.mark.parametrize("name, dtype, s, causal, pick", CASES1,
                         ids=[f"{n}-{DT_ID[dt]}-s{s}-{'causal' if c else 'full'}" for n, dt, s, c, _ in CASES1])
def test_bits_per_sequence(name, dtype, s, causal, pick):
    _check_bits(name, dtype, s, causal, pick)


def test_bits_per_sequence_bshd():
    out, _ = _check_bits("B", F16, 33, True, layout="bshd")
    assert out.shape == (len(SETS["B"][0]), 33, SETS["B"][2], SETS["B"][1])


def test_three_query_rows_take_the_prefill_route_when_asked():
    _check_bits("A", F16, 3, False)
    _check_bits("B", F16, 3, True)


# ---- 2. nothing stale is read --------------------------------------------------------------------------------------------------------
def test_nothing_stale_is_read():
    """The pool is 0xFF everywhere before the appends - the spare pages, the rows of every open page beyond its sequence's length -
    and so is the workspace: bf16 NaN wherever an image element is read that this call did not write."""
    from lqer_amd import PagedKVCache, _lib

    lens, d, h, hk = SETS["B"]
    cache = PagedKVCache(sum(map(pages_of, lens)) + 5, len(lens), hk, d, CFG, CFG, F16, DEV, max_pages_per_seq=max(map(pages_of, lens)))
    cache.buf.fill_(0xFF)
    seqs = [cache.alloc() for _ in lens]
    for sq, (k, v) in zip(seqs, _raw("B", F16)):
        cache.append([sq], k, v)
    assert cache.pages_free == 5
    for s, causal in ((129, True), (33, False)):
        ws = torch.full((_lib.lib().lqer_attention_q_paged_workspace_bytes(len(lens), h, hk, s, cache.pt.max_len, d),), 0xFF, dtype=torch.uint8, device=DEV)
        _check_bits("B", F16, s, causal, cache_seqs=(cache, seqs), ws=ws)  # (the bits of case 1, and finite)


# ---- 3. independence of the batch and of max_len ------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_or_on_max_len():
    """Sequences 0 (255 keys) and 2 (257) of set B: alone, inside the batch and inside the reversed batch, on the tight pool (the bound
    handed to the library is the table's room, 304) and on one with 200 pages per sequence (the longest addressed length rounded up to
    128: 256 resp. 384 alone, 384 in the batch) - other image strides, other grids."""
    from lqer_amd import attention_flexible_paged

    s, n = 33, len(SETS["B"][0])
    q = _q("B", F16, n, s)
    sc = q.shape[3] ** -0.5
    tight, wide = _paged("B", F16), _build("B", F16, max_pages_per_seq=200, spare=3)
    assert wide[0].pt.max_len == 3200 and tight[0].pt.max_len == 304
    for i in (0, 2):
        want, want_st = (u8(x) for x in _want("B", F16, s, True, i))
        for cache, seqs in (tight, wide):
            for order in ([i], list(range(n)), list(range(n))[::-1]):
                out, st = attention_flexible_paged(q[order], cache, [seqs[j] for j in order], sc, causal=True, return_stats=True, kernel="prefill")
                at = order.index(i)
                assert torch.equal(u8(out[at:at + 1]), want) and torch.equal(u8(st[at:at + 1]), want_st), (i, order, cache.pt.max_len)


# ---- 4. the pool is only read, the call stays inside its buffers -------------------------------------------------------------------
def test_pool_is_only_read_and_the_call_stays_inside_its_buffers():
    from lqer_amd import PagedKVCache, _lib, ops
    from lqer_amd.functional import _tri

    dt, d, h, hk, stride, s = F16, 48, 4, 2, 4, 17
    cache = PagedKVCache(9, 3, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=1, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(3, stride)  # (random bytes: a dirty pool, a dirty table)
    seqs = [cache.alloc() for _ in range(3)]
    lens = (40, 22, 18)
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t, d), dt, 3100 + i, 2.0)) for i, t in enumerate(lens)]
    for sq, (k, v) in zip(seqs, raws):
        cache.append([sq], k, v)
    q = F._randn((3, h, s, d), dt, 78, 3.0).to(DEV)
    L, f = _lib.lib(), cache.fmts
    max_len = 64  # = 16 stride: what attention_flexible_paged hands over here (40 keys rounded up to 128, capped at the table's room)
    need = L.lqer_attention_q_paged_workspace_bytes(3, h, hk, s, max_len, d)
    assert need == L.lqer_attention_q_kv_workspace_bytes(3, h, hk, s, max_len, d) > 0
    g_ws = _guard.guarded(need, align=16, fill=0xFF, name="workspace")
    g_out = _guard.guarded(q.numel() * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(3 * h * s * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(3, h, s, d), g_st.view(torch.float32).view(3, h, s, 2)
    slots = cache.pt.slots(seqs)
    torch.cuda.synchronize()
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    with torch.cuda.device(q.device):
        _lib.check(L.lqer_attention_q_paged(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, list(lens), max_len), out.data_ptr(), st.data_ptr(),
                                            ops.dtype_code(q), 3, h, hk, s, d, _tri(q), _tri(out), d ** -0.5, 1, C.byref(f[0]), C.byref(f[1]),
                                            C.byref(f[2]), C.byref(f[3]), g_ws.ptr, need, ops._stream(q.device)), "lqer_attention_q_paged")
    torch.cuda.synchronize()
    g_ws.check(), g_out.check(), g_st.check(), g_pool.check(), g_tbl.check()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)
    for b, (k, v) in enumerate(raws):
        want, want_st = _prefill(q[b:b + 1], k, v, True)
        assert torch.equal(u8(out[b:b + 1]), u8(want)) and torch.equal(u8(st[b:b + 1]), u8(want_st)), b


# ---- 5. a prompt in chunks, two sequences at once ------------------------------------------------------------------------------------
def test_prompt_in_chunks_two_sequences_at_once():
    from lqer_amd import PagedKVCache, attention_flexible_paged

    dt, d, h, hk = F16, 48, 4, 2
    have, chunks = (5, 40), (64, 64, 22)
    total = [n + sum(chunks) + 1 for n in have]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t, d), dt, 3200 + i, 2.0)) for i, t in enumerate(total)]
    cache = PagedKVCache(sum(map(pages_of, total)), 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=max(map(pages_of, total)))
    a, b = cache.alloc(), cache.alloc()
    for sq, (k, v), n in zip((a, b), raws, have):
        cache.append([sq], k[:, :, :n], v[:, :, :n])
    at = list(have)
    new = lambda x, n: torch.cat([x[i][:, :, at[i]:at[i] + n] for i in range(2)])
    for ci, n in enumerate(chunks):
        cache.append([a, b], new([r[0] for r in raws], n), new([r[1] for r in raws], n))
        at = [x + n for x in at]
        assert [cache.length(a), cache.length(b)] == at
        q = F._randn((2, h, n, d), dt, 90 + ci, 3.0).to(DEV)
        out, st = attention_flexible_paged(q, cache, [a, b], d ** -0.5, causal=True, return_stats=True, kernel="prefill")
        for i, (k, v) in enumerate(raws):
            want, want_st = _prefill(q[i:i + 1], k[:, :, :at[i]], v[:, :, :at[i]], True)
            assert torch.equal(u8(out[i:i + 1]), u8(want)) and torch.equal(u8(st[i:i + 1]), u8(want_st)), (ci, i, at[i])
    cache.append([a, b], new([r[0] for r in raws], 1), new([r[1] for r in raws], 1))  # a following single token
    q = F._randn((2, h, 1, d), dt, 99, 3.0).to(DEV)
    auto = attention_flexible_paged(q, cache, [a, b], d ** -0.5, causal=True, return_stats=True, kernel="auto")
    dec = attention_flexible_paged(q, cache, [a, b], d ** -0.5, causal=True, return_stats=True, kernel="decode")
    assert torch.equal(u8(auto[0]), u8(dec[0])) and torch.equal(u8(auto[1]), u8(dec[1]))
    q9 = F._randn((2, h, 9, d), dt, 100, 3.0).to(DEV)  # ... and beyond 8 rows "auto" is the prefill route
    auto9 = attention_flexible_paged(q9, cache, [a, b], d ** -0.5, causal=True, kernel="auto")
    pre9 = attention_flexible_paged(q9, cache, [a, b], d ** -0.5, causal=True, kernel="prefill")
    assert torch.equal(u8(auto9), u8(pre9))


# ---- 6. what the Python side refuses (nothing is launched) ---------------------------------------------------------------------------
def test_python_refusals_leave_the_pool_untouched():
    from lqer_amd import PagedKVCache, attention_flexible_paged

    dt, d, hk = F16, 48, 2
    cache = PagedKVCache(4, 4, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=2)
    a, b, c, short = (cache.alloc() for _ in range(4))
    k, v = (x.to(DEV) for x in KV._kv((1, hk, 30, d), dt, 4100))
    cache.append([a], k, v)
    cache.append([short], k[:, :, :5], v[:, :, :5])
    cache.free(c)
    torch.cuda.synchronize()
    snap, state = cache.buf.clone(), (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:])
    q = F._randn((1, 4, 20, d), dt, 5).to(DEV)
    for what, qq, seqs, kw in [("freed", q, [c], {}), ("named twice", q.repeat(2, 1, 1, 1), [a, a], {}), ("an empty sequence", q, [b], {}),
                               ("causal with s above a length", q, [short], dict(causal=True)), ("dtype", q.float(), [a], {}),
                               ("device", q.cpu(), [a], {}), ("head count", q[:, :3], [a], {}), ("head dim", q[..., :32], [a], {}),
                               ("batch", q, [a, short], {}), ("unknown kernel", q, [a], dict(kernel="flash")),
                               ("kernel=None", q, [a], dict(kernel=None))]:
        with pytest.raises(ValueError):
            attention_flexible_paged(qq, cache, seqs, 1.0, **{"kernel": "prefill", **kw})
            pytest.fail(what)
    with pytest.raises(ValueError, match="prefill"):  # the decode route still stops at 8 rows, and says where more go
        attention_flexible_paged(q, cache, [a], 1.0, kernel="decode")
    with pytest.raises(ValueError):
        attention_flexible_paged(q, cache, [a], 1.0)  # (the default)
    torch.cuda.synchronize()
    assert torch.equal(cache.buf, snap) and state == (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:])
    assert attention_flexible_paged(q, cache, [a], 1.0, kernel="prefill").shape == q.shape  # (the same call, taken)

"""Sliding-window PREFILL over the paged KV pool on the GPU (lqer_attention_q_paged_window / lqer_attention_q_paged_ragged_window:
k_attn_q's WIN instantiation of csrc/attn_q.hip on the images csrc/kv_cache.hip writes under the window;
lqer_amd.kvcache.PagedKVCache(max_query_rows=...), attention_flexible_paged(kernel="prefill", window=...), the prefill call of
attention_flexible_paged_ragged).

The contract is an equality of bits per sequence: out[b] and row_stats[b] are those of the prefill kernel's unchanged mask-tensor
instantiation on the FULL raw K and V of sequence b alone with the additive window mask - attention_flexible(q[b:b+1], K_b, V_b, ...,
attention_mask=M, kernel="prefill"), M = 0 for p - W < j <= p and torch.finfo(dtype).min elsewhere, p = i + (T_b - S_b); never paged
code - whatever the pages below the window and the workspace now hold.  Every comparison is torch.equal on the bytes; there is no
tolerance in this file.

Generators, length sets A / B / C and helpers are test_gpu_kv_window.py's.  Rows: 12 (part of a wave), 40 (two waves with a first key
each), 130 (two query tiles with a first key tile each); a call takes the set's sequences that hold at least that many keys."""
import ctypes as C
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_window as W

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES, DT_ID, u8, pages_of, SETS = W.CFG, W.DEV, W.DTYPES, W.DT_ID, W.u8, W.pages_of, W.SETS
F16 = torch.float16
WINDOWS = (1, 16, 20, 33, 70)
lo_of = lambda t, s, w: max(0, t - s - w + 1)  # the first key the call's first row sees


@functools.lru_cache(maxsize=None)
def _paged(name, dtype):
    """The set's sequences in a cache without a window (every page kept) that takes the prefill kernel's rule: the kernels' rule on its own."""
    from lqer_amd import PagedKVCache

    lens, d, _, hk = SETS[name]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens), hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=max(map(pages_of, lens)), max_query_rows=130)
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v) in zip(seqs, W._raw(name, dtype)):
        cache.append([s], k, v)
    return cache, seqs


@functools.lru_cache(maxsize=None)
def _want_cached(name, dtype, i, s, w, seed):
    q1 = _q(name, dtype, s, seed)[i:i + 1]
    return _want(q1, *W._raw(name, dtype)[i], w)


def _want(q1, k, v, w):
    """The comparator: the prefill kernel's mask-tensor instantiation on the full raw tensors of ONE sequence."""
    from lqer_amd import attention_flexible

    t, s = k.shape[2], q1.shape[2]
    return attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, attention_mask=W._mask(t, s, w, q1.dtype), kernel="prefill", return_stats=True)


@functools.lru_cache(maxsize=None)
def _q(name, dtype, s, seed=11):
    """Queries for every sequence of the set (a call picks its rows), made once."""
    lens, d, h, _ = SETS[name]
    return W._q(d, h, dtype, len(lens), s, seed)


def _same(got, got_st, want, want_st, what):
    assert got.shape == want.shape and got_st.shape == want_st.shape, what
    assert torch.equal(u8(got), u8(want)), f"{what}: {(got != want).sum().item()} of {want.numel()} outputs differ"
    assert torch.equal(u8(got_st), u8(want_st)), f"{what}: row_stats differ"


def _check_bits(cache, seqs, raws, q, w, what="", explicit=True, kernel="prefill", ws=None):
    """out[b] and stats[b] of one windowed call over `seqs` against the comparator on raws[b], for every b."""
    from lqer_amd import attention_flexible_paged

    out, st = attention_flexible_paged(q, cache, seqs, q.shape[3] ** -0.5, causal=True, return_stats=True, kernel=kernel, ws=ws,
                                       **({"window": w} if explicit else {}))
    assert out.dtype == q.dtype and st.shape == (*q.shape[:3], 2)
    for b, (k, v) in enumerate(raws):
        _same(out[b:b + 1], st[b:b + 1], *_want(q[b:b + 1], k, v, w), f"{what} sequence {b} ({k.shape[2]} keys, {q.shape[2]} rows, window {w})")
    assert torch.isfinite(out).all()
    return out, st


# ---- 1. the rule, on pools that still hold every page ---------------------------------------------------------------------------------
CASES = ([("A", dt, w, s) for dt in DTYPES for w in WINDOWS for s in (12, 40)]
         + [(n, F16, w, s) for n in ("B", "C") for w in WINDOWS for s in (12, 40, 130)])


@pytest.mark.parametrize("name, dtype, w, s", CASES, ids=[f"{n}-{DT_ID[dt]}-w{w}-s{s}" for n, dt, w, s in CASES])
def test_bits_per_sequence(name, dtype, w, s):
    from lqer_amd import attention_flexible_paged

    cache, seqs = _paged(name, dtype)
    lens = SETS[name][0]
    pick = [i for i, n in enumerate(lens) if n >= s]
    assert pick and max(lens[i] for i in pick) > w  # (the windowed entry runs)
    q = _q(name, dtype, s)[pick]
    out, st = attention_flexible_paged(q, cache, [seqs[i] for i in pick], q.shape[3] ** -0.5, causal=True, return_stats=True, kernel="prefill", window=w)
    for b, i in enumerate(pick):
        _same(out[b:b + 1], st[b:b + 1], *_want_cached(name, dtype, i, s, w, 11), f"sequence {i} ({lens[i]} keys, {s} rows, window {w})")
    assert torch.isfinite(out).all()


def test_head_dim_128():
    """DK = 4 (d = 48, 64, 16 above are DK = 2, 2, 1; d = 96 here is DK = 3): 300 keys, 130 rows, W = 33."""
    from lqer_amd import PagedKVCache

    for d, seed in ((128, 7000), (96, 7010)):
        k, v = W._kv(300, d, 2, F16, seed)
        cache = PagedKVCache(19, 1, 2, d, CFG, CFG, F16, DEV, max_pages_per_seq=19, max_query_rows=130)
        s = cache.alloc()
        cache.append([s], k, v)
        _check_bits(cache, [s], [(k, v)], W._q(d, 4, F16, 1, 130, seed=3), 33, what=f"d = {d}:")


def test_the_cases_reach_the_edges_they_are_there_for():
    """Host arithmetic of the rule: lo = max(0, T - S - W + 1); the images are written from tile lo // 64 on, pages below lo // 16 are
    not read, and the workgroup of query tile q0 starts at tile max(0, q0 + T - S - W + 1) // 64."""
    assert lo_of(100, 12, 20) == 69 and 69 % 16 == 5                                    # A: inside a page
    assert lo_of(257, 12, 70) == 176 and 176 % 16 == 0 and 176 % 64                     # B: on a page edge, inside a tile
    assert lo_of(300, 12, 33) == 256 and 256 % 64 == 0                                   # B: on a 64-key tile edge
    assert lo_of(257, 12, 1) // 64 == 3 and lo_of(2049, 130, 70) // 64 == 28            # B, C: at least two dead tiles below it
    assert lo_of(100, 12, 1) == 88 and (88 // 16) % 4 == 1                              # A: the first live tile (64 ..) holds page 4 dead, page 5 live
    assert lo_of(300, 12, 1) == 288 and (288 // 16) % 4 == 2                            # B: ... two dead pages, on a page edge
    assert lo_of(100, 40, 70) == 0 and lo_of(37, 12, 33) == 0                           # nothing dead: the rule cuts rows, not the first one
    # 40 rows: the second wave's first key lies 32 beyond the first's; 130 rows: the second query tile's first key tile is another
    assert (lo_of(300, 130, 16) + 128) // 64 != lo_of(300, 130, 16) // 64 and (lo_of(2049, 130, 70) + 128) // 64 == 30


# ---- 2. W >= T is plain causal --------------------------------------------------------------------------------------------------------------
def _c_call(cache, seqs, q, w, max_len=None, ws=None, out=None, st=None):
    """lqer_attention_q_paged_window as it stands, whatever W is (the Python route takes the unwindowed entry while every length <= W)."""
    from lqer_amd import _lib, ops
    from lqer_amd.kvcache import _tri

    L, f = _lib.lib(), cache.fmts
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    b, h, s, d = q.shape
    max_len = min((max(lens) + 127) // 128 * 128, cache.pt.max_len) if max_len is None else max_len
    out = torch.empty_like(q) if out is None else out
    st = torch.empty(b, h, s, 2, dtype=torch.float32, device=DEV) if st is None else st
    if ws is None:
        ws = torch.full((L.lqer_attention_q_paged_workspace_bytes(b, h, cache.kv_heads, s, max_len, d),), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(q.device):
        _lib.check(L.lqer_attention_q_paged_window(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(), st.data_ptr(),
                                                   ops.dtype_code(q), b, h, cache.kv_heads, s, d, _tri(q), _tri(out), d ** -0.5, 1, C.byref(f[0]),
                                                   C.byref(f[1]), C.byref(f[2]), C.byref(f[3]), ws.data_ptr(), ws.numel(), ops._stream(q.device), w),
                   "lqer_attention_q_paged_window")
    return out, st


def _c_ragged(cache, seqs, counts, q, w, max_len=None, ws=None, out=None, st=None):
    """lqer_attention_q_paged_ragged_window as it stands: q / out [sum(counts), h, d]."""
    from lqer_amd import _lib, ops
    from lqer_amd.kvcache import _pair

    L, f = _lib.lib(), cache.fmts
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    total, h, d = q.shape
    max_len = min((max(lens) + 127) // 128 * 128, cache.pt.max_len) if max_len is None else max_len
    out = torch.empty_like(q) if out is None else out
    st = torch.empty(total, h, 2, dtype=torch.float32, device=DEV) if st is None else st
    if ws is None:
        ws = torch.full((L.lqer_attention_q_paged_ragged_workspace_bytes(len(seqs), h, cache.kv_heads, max(counts), max_len, d),), 0xFF, dtype=torch.uint8,
                        device=DEV)
    with torch.cuda.device(q.device):
        _lib.check(L.lqer_attention_q_paged_ragged_window(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(),
                                                          st.data_ptr(), ops.dtype_code(q), len(seqs), h, cache.kv_heads, cache._call_starts(counts),
                                                          max(counts), total, d, _pair(q), _pair(out), d ** -0.5, 1, C.byref(f[0]), C.byref(f[1]),
                                                          C.byref(f[2]), C.byref(f[3]), ws.data_ptr(), ws.numel(), ops._stream(q.device), w),
                   "lqer_attention_q_paged_ragged_window")
    return out, st


@pytest.mark.parametrize("name, s", [("A", 12), ("B", 130)])
def test_a_window_that_covers_everything_is_plain_causal(name, s):
    from lqer_amd import attention_flexible_paged

    cache, seqs = _paged(name, F16)
    lens, d, h, _ = SETS[name]
    q = _q(name, F16, s)
    out, st = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True, kernel="prefill")  # window=None on a cache without one
    for w in (max(lens), max(lens) + 1, 1 << 40, 1 << 62):
        wout, wst = _c_call(cache, seqs, q, w)
        assert torch.equal(u8(wout), u8(out)) and torch.equal(u8(wst), u8(st)), w
        pout, pst = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True, kernel="prefill", window=min(w, 1 << 40))
        assert torch.equal(u8(pout), u8(out)) and torch.equal(u8(pst), u8(st)), w
    # W between the lengths: the windowed entry runs, and the sequences it covers whole get the plain causal bits
    w = sorted(lens)[-2]
    wout, wst = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True, kernel="prefill", window=w)
    whole = [i for i, n in enumerate(lens) if n <= w]
    assert whole and len(whole) < len(lens)
    assert torch.equal(u8(wout[whole]), u8(out[whole])) and torch.equal(u8(wst[whole]), u8(st[whole]))
    assert not torch.equal(u8(wout), u8(out))


# ---- 3. released pages are never read ----------------------------------------------------------------------------------------------------------
def _packed(qs):
    """[1, h, c, d] each -> [sum(c), h, d]."""
    return torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous()


def _check_ragged(cache, seqs, raws, counts, w, kernel, what="", seed=61, explicit=False, ws=None):
    """One attention_flexible_paged_ragged call: every sequence's rows against the comparator of the route it takes - the decode
    kernel's (test_gpu_kv_window.py's) for up to 8 rows under "auto", the prefill kernel's beyond."""
    from lqer_amd import attention_flexible_paged_ragged

    d, h = cache.head_dim, 4
    qs = [W._q(d, h, cache.dtype, 1, c, seed=seed + b) if c else None for b, c in enumerate(counts)]
    q = _packed([x for x in qs if x is not None])
    out, st = attention_flexible_paged_ragged(q, cache, seqs, counts, d ** -0.5, causal=True, return_stats=True, kernel=kernel, ws=ws,
                                              **({"window": w} if explicit else {}))
    at = 0
    for b, (c, raw) in enumerate(zip(counts, raws)):
        if not c:
            continue
        want, want_st = (W._want if kernel == "auto" and c <= 8 else _want)(qs[b], *raw, w)
        _same(out[at:at + c], st[at:at + c], want[0].transpose(0, 1), want_st[0].transpose(0, 1), f"{what} sequence {b} ({raw[0].shape[2]} keys, {c} rows, window {w})")
        at += c
    assert torch.isfinite(out).all()
    return q, out, st


def _released_cache(dtype, w=20, rows=40, lens=(37, 90, 100, 300), steps=(7, 33, 40, 40), d=48, hk=2, spare_seqs=1, seed=6000):
    """Sequences grown by chunks of up to `rows` keys in a window=w, max_query_rows=rows cache: their old pages went back on the way."""
    from lqer_amd import PagedKVCache

    raws = [W._kv(n, d, hk, dtype, seed + i) for i, n in enumerate(lens)]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens) + spare_seqs, hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=24, window=w, max_query_rows=rows)
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v), step in zip(seqs, raws, steps):
        W._grow(cache, s, k, v, step)
    return cache, seqs, raws


@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
def test_released_pages_are_never_read(dtype):
    """W = 20, R = 40: the old pages go back to the pool during the appends; another sequence then takes every freed page and writes
    keys with larger exponents there.  The workspace starts as 0xFF bytes - a NaN in every stale image row.  The bits still are the
    comparator's, and every output is finite."""
    w, rows, lens = 20, 40, (37, 90, 100, 300)
    cache, seqs, raws = _released_cache(dtype)
    d, h, hk = 48, 4, 2
    gone = [cache.pt.released[cache.pt.slot(s)] for s in seqs]
    assert gone == [0, 1, 2, 15] and cache.pages_free == sum(gone)
    assert all(16 * g <= lo_of(n, rows, w) for g, n in zip(gone, lens))
    stale = {p for s, g in zip(seqs, gone) for p in cache.pt.table[cache.pt.slot(s)][:g]}
    held = {p for s, g in zip(seqs, gone) for p in cache.pt.table[cache.pt.slot(s)][g:cache.pt.pages_of[cache.pt.slot(s)]]}
    other, n_other = cache.alloc(), 16 * cache.pages_free
    ko, vo = W._kv(n_other, d, hk, dtype, 6100)
    cache.append([other], 64 * ko, 64 * vo)  # larger exponents everywhere (one append from empty: nothing of it is released)
    mine = set(cache.pt.table[cache.pt.slot(other)][:pages_of(n_other)])
    assert cache.pages_free == 0 and len(mine) == sum(gone) and not mine & held and stale <= mine | held and stale & mine
    ws = lambda: torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=DEV)
    for s_rows in (12, 33):
        _check_bits(cache, seqs, raws, W._q(d, h, dtype, len(seqs), s_rows, seed=23), w, what="after release:", explicit=False, ws=ws())
    _check_bits(cache, seqs[1:], raws[1:], W._q(d, h, dtype, 3, 40, seed=24), w, what="after release, R rows:", explicit=False, kernel="auto", ws=ws())
    _check_bits(cache, seqs, raws, W._q(d, h, dtype, len(seqs), 12, seed=29), 9, what="a narrower window:", ws=ws())
    _check_ragged(cache, seqs, raws, (12, 40, 9, 40), w, "prefill", what="ragged, after release:", ws=ws())


# ---- 4. a prompt in chunks, in a pool of the bound's size --------------------------------------------------------------------------------------------
def test_a_prompt_in_chunks_in_a_pool_of_the_bounds_size():
    """300 keys in chunks of 32 (the last: 12) to two sequences, W = 20, R = 32, in a pool of exactly 2 ((W + R + 29) // 16) pages - the most two
    sequences can hold -: never out of pages, and every chunk's bits are the comparator's on the raw history so far."""
    from lqer_amd import PagedKVCache

    w, rows, d, h, hk, n, dt = 20, 32, 48, 4, 2, 300, F16
    bound = (w + rows + 29) // 16
    raws = [W._kv(n, d, hk, dt, 6200 + i) for i in range(2)]
    cache = PagedKVCache(2 * bound, 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=pages_of(n), window=w, max_query_rows=rows)
    seqs = [cache.alloc(), cache.alloc()]
    most = 0
    for at in range(0, n, rows):
        c = min(rows, n - at)
        cache.append(seqs, torch.cat([k[:, :, at:at + c] for k, _ in raws]), torch.cat([v[:, :, at:at + c] for _, v in raws]))
        held = [cache.pages_held(s) for s in seqs]
        assert max(held) <= bound and cache.pages_free == 2 * bound - sum(held)
        most = max(most, *held)
        t = at + c
        _check_bits(cache, seqs, [(k[:, :, :t], v[:, :, :t]) for k, v in raws], W._q(d, h, dt, 2, c, seed=40 + at), w, what=f"chunk at {at}:", explicit=False,
                    kernel="auto")
    assert most <= bound and [cache.pt.released[cache.pt.slot(s)] for s in seqs] == [(n - w - (rows - 1)) // 16] * 2


# ---- 5. one ragged step ----------------------------------------------------------------------------------------------------------------------------------
def test_one_ragged_step_on_released_sequences():
    """Counts [1, 3, 12, 40, 0] under kernel="auto": the decoders in one windowed decode call, the chunks in one windowed prefill call,
    and each sequence's bits are those of the call on it alone."""
    from lqer_amd import attention_flexible_paged, attention_flexible_paged_ragged

    w, counts = 20, (1, 3, 12, 40, 0)
    cache, seqs, raws = _released_cache(F16, lens=(80, 100, 90, 300, 76), steps=(40, 33, 40, 40, 25), spare_seqs=0, seed=6500)
    assert all(cache.pt.released[cache.pt.slot(s)] for s in seqs)
    plan = attention_flexible_paged_ragged.plan(cache, seqs, counts)
    assert [(p["call"], p["seqs"], p["window"]) for p in plan] == [("lqer_attention_q_decode_paged_ragged", [0, 1], w),
                                                                 ("lqer_attention_q_paged_ragged_window", [2, 3], w)]
    q, out, st = _check_ragged(cache, seqs, raws, counts, w, "auto", what="ragged step:")
    at = 0
    for s, c in zip(seqs, counts):
        if c:
            q1 = q[at:at + c].transpose(0, 1).unsqueeze(0)
            alone, alone_st = attention_flexible_paged(q1, cache, [s], 48 ** -0.5, causal=True, return_stats=True, kernel="auto")
            _same(out[at:at + c], st[at:at + c], alone[0].transpose(0, 1), alone_st[0].transpose(0, 1), f"sequence {s} alone")
        at += c
    # kernel="prefill": the whole step in one windowed call, 1 and 3 rows on the prefill kernel too
    _check_ragged(cache, seqs, raws, counts, w, "prefill", what="ragged step, one call:")


# ---- 6. independence of the batch and of max_len ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, s, w, wide", [("A", 12, 20, 40), ("B", 130, 33, 200)])
def test_rows_do_not_depend_on_the_batch_or_on_max_len(name, s, w, wide):
    """`wide` pages per sequence and max_len = 16 wide: other image strides, other grids."""
    from lqer_amd import PagedKVCache

    cache, seqs = _paged(name, F16)
    lens, d, h, hk = SETS[name]
    pick = [i for i, n in enumerate(lens) if n >= s]
    q = _q(name, F16, s)[pick]
    out, st = _c_call(cache, [seqs[i] for i in pick], q, w)
    for b, i in enumerate(pick):
        _same(out[b:b + 1], st[b:b + 1], *_want_cached(name, F16, i, s, w, 11), f"sequence {i}")
    order = list(range(len(pick)))[::-1]
    sub, sub_st = _c_call(cache, [seqs[pick[j]] for j in order], q[order], w)
    assert torch.equal(u8(sub), u8(out[order])) and torch.equal(u8(sub_st), u8(st[order]))
    one, one_st = _c_call(cache, [seqs[pick[-1]]], q[-1:], w)
    assert torch.equal(u8(one), u8(out[-1:])) and torch.equal(u8(one_st), u8(st[-1:]))
    big = PagedKVCache(sum(map(pages_of, lens)) + 3, len(lens), hk, d, CFG, CFG, F16, DEV, max_pages_per_seq=wide, window=w, max_query_rows=max(s, 8))
    big_seqs = [big.alloc() for _ in lens]
    for sq, (k, v) in zip(big_seqs, W._raw(name, F16)):
        W._grow(big, sq, k, v, 8)  # (and its old pages released on the way)
    assert big.pt.max_len == 16 * wide > cache.pt.max_len and big.pages_free > 3
    wout, wst = _c_call(big, [big_seqs[i] for i in pick], q, w, max_len=16 * wide)
    assert torch.equal(u8(wout), u8(out)) and torch.equal(u8(wst), u8(st))
    # the ragged entry with every count = s is the same call
    rout, rst = _c_ragged(big, [big_seqs[i] for i in pick], [s] * len(pick), _packed([q[b:b + 1] for b in range(len(pick))]), w, max_len=16 * wide)
    assert torch.equal(u8(rout), u8(_packed([out[b:b + 1] for b in range(len(pick))])))
    assert torch.equal(u8(rst), u8(_packed([st[b:b + 1] for b in range(len(pick))])))


# ---- 7. footprint --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["uniform", "ragged"])
def test_footprint(entry):
    """q is a guarded input; out, statistics, workspace (0xFF), pool and table carry guard zones; the attention writes nothing of the
    pool, and nothing outside what it was given."""
    from lqer_amd import PagedKVCache, _lib

    w, rows, dt, d, h, hk, stride = 20, 40, F16, 48, 4, 2, 12
    lens, steps = (80, 100, 180), (40, 33, 40)
    counts = (40, 40, 40) if entry == "uniform" else (12, 40, 9)
    cache = PagedKVCache(sum(map(pages_of, lens)), 3, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride, window=w, max_query_rows=rows)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=0xFF, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(3, stride)
    seqs = [cache.alloc() for _ in lens]
    raws = [W._kv(n, d, hk, dt, 6600 + i) for i, n in enumerate(lens)]
    for s, (k, v), step in zip(seqs, raws, steps):
        W._grow(cache, s, k, v, step)
    assert all(cache.pt.released[cache.pt.slot(s)] for s in seqs)
    qs = [F._randn((1, h, c, d), dt, 90 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    total, max_len = sum(counts), 16 * stride
    L = _lib.lib()
    if entry == "uniform":
        qt, need = torch.cat(qs), L.lqer_attention_q_paged_workspace_bytes(3, h, hk, counts[0], max_len, d)
        oshape, sshape = (3, h, counts[0], d), (3, h, counts[0], 2)
    else:
        qt, need = _packed(qs), L.lqer_attention_q_paged_ragged_workspace_bytes(3, h, hk, max(counts), max_len, d)
        oshape, sshape = (total, h, d), (total, h, 2)
    g_q = _guard.guarded(qt.numel() * 2, align=16, name="q").load(qt)
    g_ws = _guard.guarded(need, align=16, fill=0xFF, name="workspace")
    g_out = _guard.guarded(qt.numel() * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(total * h * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(oshape), g_st.view(torch.float32).view(sshape)
    torch.cuda.synchronize()
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    if entry == "uniform":
        _c_call(cache, seqs, g_q.view(dt).view(oshape), w, max_len=max_len, ws=g_ws.payload, out=out, st=st)
    else:
        _c_ragged(cache, seqs, counts, g_q.view(dt).view(oshape), w, max_len=max_len, ws=g_ws.payload, out=out, st=st)
    torch.cuda.synchronize()
    g_ws.check(), g_out.check(), g_st.check(), g_pool.check(), g_tbl.check(), g_q.unchanged()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)
    at = 0
    for b, ((k, v), c) in enumerate(zip(raws, counts)):
        want, want_st = _want(qs[b], k, v, w)
        if entry == "uniform":
            _same(out[b:b + 1], st[b:b + 1], want, want_st, f"sequence {b}")
        else:
            _same(out[at:at + c], st[at:at + c], want[0].transpose(0, 1), want_st[0].transpose(0, 1), f"sequence {b}")
        at += c
    assert torch.isfinite(out).all()

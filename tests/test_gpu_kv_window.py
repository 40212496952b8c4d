"""Sliding-window attention over the paged KV pool on the GPU (lqer_attention_q_decode_paged_window: k_attn_dec_scores / k_attn_dec_pv /
k_attn_dec_sum of csrc/attn_decode.hip with the window rule; lqer_amd.kvcache.PagedKVCache(window=...), attention_flexible_paged(window=...)).

The contract is an equality of bits per sequence: out[b] and row_stats[b] of one windowed call are those of the decode kernel on the
FULL raw K and V of sequence b alone with the additive window mask - attention_flexible(q[b:b+1], K_b, V_b, ..., attention_mask=M,
kernel="decode"), M = 0 for p - W < j <= p and torch.finfo(dtype).min elsewhere, p = i + (T_b - S); never the paged code itself -
whatever the pages below the window now hold.  Every comparison is torch.equal on the bytes; there is no tolerance in this file.

Length sets, the smallest that reach every edge of the rule:
  A (17, 37, 70, 100)  D 48, heads 4 / 2, chunks of 16 = one page: dead chunks, the window's edge inside a page, an edge per query row;
  B (257, 300)         D 64, heads 8 / 2, chunks of 32: at W = 40 the first live chunk of the 257 holds one dead and one live page;
  C (2049, 5)          D 16, heads 2 / 1, chunks of 128: at W = 200 14 dead chunks, then a chunk of 8 pages of which 3 are dead, and a
                       sequence whose window is a no-op in the same grid."""
import functools

import pytest
import torch

import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
import test_gpu_kv_paged as P

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES, DT_ID, u8, pages_of = P.CFG, P.DEV, P.DTYPES, P.DT_ID, P.u8, P.pages_of
SETS = {"A": ((17, 37, 70, 100), 48, 4, 2), "B": ((257, 300), 64, 8, 2), "C": ((2049, 5), 16, 2, 1)}  # lengths, d, h, hk


def _kv(n, d, hk, dtype, seed):
    return tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dtype, seed, 2.0))


@functools.lru_cache(maxsize=None)
def _raw(name, dtype):
    """The raw K and V of the set's sequences, [1, hk, L, d] each, on the device: made once, shared, never written."""
    lens, d, _, hk = SETS[name]
    return tuple(_kv(n, d, hk, dtype, 5000 + 16 * i + ord(name)) for i, n in enumerate(lens))


@functools.lru_cache(maxsize=None)
def _paged(name, dtype):
    """The set's sequences in a cache WITHOUT a window (every page kept): the kernels' rule on its own."""
    from lqer_amd import PagedKVCache

    lens, d, _, hk = SETS[name]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens), hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=max(map(pages_of, lens)))
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v) in zip(seqs, _raw(name, dtype)):
        cache.append([s], k, v)
    return cache, seqs


def _mask(t, s, w, dtype):
    """[1, 1, s, t]: 0 where query row i (position p = i + t - s) sees key j, p - w < j <= p; the most negative finite value elsewhere."""
    p = torch.arange(s).view(s, 1) + (t - s)
    j = torch.arange(t).view(1, t)
    m = torch.zeros(s, t, dtype=dtype)
    m[~((j <= p) & (j > p - w))] = torch.finfo(dtype).min
    return m.view(1, 1, s, t).to(DEV)


def _want(q1, k, v, w):
    """The comparator: the decode kernel on the full raw tensors of ONE sequence with the window as a mask tensor."""
    from lqer_amd import attention_flexible

    t, s = k.shape[2], q1.shape[2]
    return attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, attention_mask=_mask(t, s, w, q1.dtype), kernel="decode", return_stats=True)


def _check_bits(cache, seqs, raws, q, w, what="", explicit=True):
    """out[b] and stats[b] of one windowed call over `seqs` against the comparator on raws[b], for every b."""
    from lqer_amd import attention_flexible_paged

    out, st = attention_flexible_paged(q, cache, seqs, q.shape[3] ** -0.5, causal=True, return_stats=True, **({"window": w} if explicit else {}))
    assert out.dtype == q.dtype and st.shape == (*q.shape[:3], 2)
    for b, (k, v) in enumerate(raws):
        want, want_st = _want(q[b:b + 1], k, v, w)
        assert torch.equal(u8(out[b:b + 1]), u8(want)), \
            f"{what} sequence {b} ({k.shape[2]} keys, window {w}): {(out[b:b + 1] != want).sum().item()} of {want.numel()} outputs differ"
        assert torch.equal(u8(st[b:b + 1]), u8(want_st)), f"{what} sequence {b} ({k.shape[2]} keys, window {w}): row_stats differ"
    assert torch.isfinite(out).all()
    return out, st


def _q(d, h, dtype, n, s, seed=11):
    return F._randn((n, h, s, d), dtype, seed + s, 3.0).to(DEV)


# ---- 1 - 3. the rule, on pools that still hold every page ---------------------------------------------------------------------------
CASES = ([("A", dt, w, s) for dt in DTYPES for w in (1, 16, 20, 33) for s in (1, 3, 8)]
         + [("B", torch.float16, w, s) for w in (40, 250) for s in (1, 3, 8)]
         + [("C", torch.float16, 200, s) for s in (1, 3, 5)])  # (the short sequence of C has 5 keys: causal takes up to 5 rows)


@pytest.mark.parametrize("name, dtype, w, s", CASES, ids=[f"{n}-{DT_ID[dt]}-w{w}-s{s}" for n, dt, w, s in CASES])
def test_bits_per_sequence(name, dtype, w, s):
    cache, seqs = _paged(name, dtype)
    _, d, h, _ = SETS[name]
    _check_bits(cache, seqs, _raw(name, dtype), _q(d, h, dtype, len(seqs), s), w)


def test_the_sets_reach_the_edges_they_are_there_for():
    """Host arithmetic of the kernels' rule: lo = max(0, T - S - W + 1), dead chunks below lo // C, dead pages below lo // 16."""
    chunk = lambda t: 16 * min(max((t + 255) // 256, 1), 8)
    lo = lambda t, s, w: max(0, t - s - w + 1)
    assert chunk(100) == 16 and lo(100, 1, 33) // 16 == 4 and lo(100, 1, 33) % 16 == 3           # A: dead chunks, the edge inside a page
    assert lo(100, 1, 20) % 16 == 0 and lo(100, 8, 33) // 16 == 3                                # ... on a page's edge; the first of 8 rows a page earlier
    assert chunk(257) == 32 and lo(257, 1, 40) // 32 == 6 and lo(257, 1, 40) // 16 == 13         # B: chunk 6 = pages 12 (dead) and 13
    assert chunk(2049) == 128 and lo(2049, 1, 200) // 128 == 14 and (lo(2049, 1, 200) // 16) % 8 == 3  # C: 14 dead chunks, 3 dead pages of 8
    assert chunk(2049) == 128 and lo(2049, 5, 200) // 128 == 14 and lo(5, 5, 200) == 0


# ---- 4. W >= T is plain causal ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_a_window_that_covers_everything_is_plain_causal(name):
    from lqer_amd import attention_flexible_paged

    dt = torch.float16
    cache, seqs = _paged(name, dt)
    lens, d, h, _ = SETS[name]
    q = _q(d, h, dt, len(seqs), 3)
    out, st = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True)  # window=None on a cache without one
    for w in (max(lens), max(lens) + 1, 1 << 40):
        wout, wst = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True, window=w)
        assert torch.equal(u8(wout), u8(out)) and torch.equal(u8(wst), u8(st)), w


# ---- 5. released pages are never read -----------------------------------------------------------------------------------------------------
def _grow(cache, seq, k, v, step, at=0, upto=None):
    upto = k.shape[2] if upto is None else upto
    while at < upto:
        n = min(step, upto - at)
        cache.append([seq], k[:, :, at:at + n], v[:, :, at:at + n])
        at += n


@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
def test_released_pages_are_never_read(dtype):
    """The sequences grow in a cache with W = 20, so their old pages go back to the pool during the appends; another sequence then takes
    every freed page and writes other data there.  The stale entries of the windowed sequences' rows name those pages - valid
    indices, other contents - and the bits still are the comparator's.  300 keys: chunks of 32, and the first live chunk holds the
    released page of keys 256 .. 271 next to a live one."""
    from lqer_amd import PagedKVCache

    w, d, h, hk, lens = 20, 48, 4, 2, (37, 70, 100, 300)
    raws = [_kv(n, d, hk, dtype, 6000 + i) for i, n in enumerate(lens)]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens) + 1, hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=24, window=w)  # (24: the 23 freed pages in one row)
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v), step in zip(seqs, raws, (1, 5, 8, 7)):
        _grow(cache, s, k, v, step)
    gone = [cache.pt.released[cache.pt.slot(s)] for s in seqs]
    assert gone == [max(0, (n - w - 7) // 16) for n in lens] == [0, 2, 4, 17] and cache.pages_free == sum(gone)
    stale = {p for s, g in zip(seqs, gone) for p in cache.pt.table[cache.pt.slot(s)][:g]}
    held = {p for s, g in zip(seqs, gone) for p in cache.pt.table[cache.pt.slot(s)][g:cache.pt.pages_of[cache.pt.slot(s)]]}
    other, n_other = cache.alloc(), 16 * cache.pages_free
    ko, vo = _kv(n_other, d, hk, dtype, 6100)
    cache.append([other], 64 * ko, 64 * vo)  # larger exponents everywhere
    mine = set(cache.pt.table[cache.pt.slot(other)][:pages_of(n_other)])
    # every page that was ever let go is in use again - by the other sequence, or by a windowed one that grew later (the 300 keys took
    # what the shorter ones and it itself had freed) - so every stale entry names a page that now holds other keys
    assert cache.pages_free == 0 and len(mine) == sum(gone) and not mine & held and stale <= mine | held and stale & mine
    for s_rows in (1, 3, 8):
        _check_bits(cache, seqs, raws, _q(d, h, dtype, len(seqs), s_rows, seed=23), w, what="after release:", explicit=False)
    _check_bits(cache, seqs, raws, _q(d, h, dtype, len(seqs), 2, seed=29), 9, what="a narrower window:")
    # the other sequence is one like any other (its window: the last 20 of its keys)
    _check_bits(cache, [other], [(64 * ko, 64 * vo)], _q(d, h, dtype, 1, 3, seed=31), w, explicit=False)


# ---- 6. growth by decode steps in a pool sized for the window ---------------------------------------------------------------------------------
def test_decode_steps_in_a_pool_of_the_windows_size():
    """80 one-key appends to two sequences, W = 20, in a pool of exactly 2 ((W + 37) // 16) pages: never out of pages, and every step's
    bits are the comparator's on the raw history so far (1, 3 and 8 query rows in turn)."""
    from lqer_amd import PagedKVCache

    w, d, h, hk, steps, dt = 20, 48, 4, 2, 80, torch.float16
    bound = (w + 37) // 16
    raws = [_kv(steps, d, hk, dt, 6200 + i) for i in range(2)]
    cache = PagedKVCache(2 * bound, 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=pages_of(steps), window=w)
    seqs = [cache.alloc(), cache.alloc()]
    most = 0
    for t in range(1, steps + 1):
        cache.append(seqs, torch.cat([k[:, :, t - 1:t] for k, _ in raws]), torch.cat([v[:, :, t - 1:t] for _, v in raws]))
        held = [cache.pages_held(s) for s in seqs]
        assert max(held) <= bound and cache.pages_free == 2 * bound - sum(held)
        most = max(most, *held)
        s_rows = min((1, 3, 8)[t % 3], t)
        _check_bits(cache, seqs, [(k[:, :, :t], v[:, :, :t]) for k, v in raws], _q(d, h, dt, 2, s_rows, seed=40 + t), w, what=f"step {t}:", explicit=False)
    assert most == bound and [cache.pt.released[cache.pt.slot(s)] for s in seqs] == [(steps - w - 7) // 16] * 2


# ---- 7. forks of a trimmed sequence ---------------------------------------------------------------------------------------------------------------
def test_fork_of_a_trimmed_sequence():
    from lqer_amd import PagedKVCache

    w, d, h, hk, dt = 20, 48, 4, 2, torch.float16
    kp, vp = _kv(70 + 45, d, hk, dt, 6300)  # the parent's history: 70 keys before the fork, 45 after
    kc, vc = _kv(45, d, hk, dt, 6310)       # the child's own continuation
    cache = PagedKVCache(12, 3, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=8, window=w)
    parent = cache.alloc()
    _grow(cache, parent, kp, vp, 8, upto=70)
    assert cache.pt.released[cache.pt.slot(parent)] == 2 and cache.pages_free == 12 - 3
    child, = cache.fork(parent)
    assert cache.pt.released[cache.pt.slot(child)] == 2 and cache.pages_shared == 2 and cache.pages_free == 12 - 4  # pages 2, 3 shared; the open block copied
    child_k, child_v = torch.cat([kp[:, :, :70], kc], 2), torch.cat([vp[:, :, :70], vc], 2)
    for at in range(0, 45, 5):  # in turn: each releases shared pages on its own, the page goes back with the second owner
        cache.append([parent], kp[:, :, 70 + at:75 + at], vp[:, :, 70 + at:75 + at])
        cache.append([child], kc[:, :, at:at + 5], vc[:, :, at:at + 5])
        t = 75 + at
        raws = [(kp[:, :, :t], vp[:, :, :t]), (child_k[:, :, :t], child_v[:, :, :t])]
        _check_bits(cache, [parent, child], raws, _q(d, h, dt, 2, 3, seed=50 + at), w, what=f"fork, {t} keys:", explicit=False)
    assert cache.pages_shared == 0 and all(cache.pages_held(s) <= (w + 37) // 16 for s in (parent, child))
    cache.free(parent)
    _check_bits(cache, [child], [(child_k, child_v)], _q(d, h, dt, 1, 8, seed=70), w, what="fork, parent freed:", explicit=False)
    cache.free(child)
    assert cache.pages_free == 12 and cache.pt._owners.tolist() == [0] * 12


# ---- 8. independence of the batch and of max_len ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, wide, w", [("A", 40, 20), ("B", 200, 40)])
def test_rows_do_not_depend_on_the_batch_or_on_max_len(name, wide, w):
    """`wide` pages per sequence: 640 resp. 3200 keys of max_len - other workspace strides, a grid of 16 resp. 25 chunks."""
    from lqer_amd import PagedKVCache, attention_flexible_paged

    dt = torch.float16
    cache, seqs = _paged(name, dt)
    lens, d, h, hk = SETS[name]
    q = _q(d, h, dt, len(seqs), 3)
    out, st = attention_flexible_paged(q, cache, seqs, d ** -0.5, causal=True, return_stats=True, window=w)
    pick = [1, 0]
    sub, sub_st = attention_flexible_paged(q[pick], cache, [seqs[i] for i in pick], d ** -0.5, causal=True, return_stats=True, window=w)
    assert torch.equal(u8(sub), u8(out[pick])) and torch.equal(u8(sub_st), u8(st[pick]))
    big = PagedKVCache(sum(map(pages_of, lens)) + 3, len(lens), hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=wide, window=w)
    big_seqs = [big.alloc() for _ in lens]
    for s, (k, v) in zip(big_seqs, _raw(name, dt)):
        _grow(big, s, k, v, 8)  # (and its old pages released on the way)
    assert big.pt.max_len == 16 * wide > cache.pt.max_len and big.pages_free > 3
    wout, wst = attention_flexible_paged(q, big, big_seqs, d ** -0.5, causal=True, return_stats=True)
    assert torch.equal(u8(wout), u8(out)) and torch.equal(u8(wst), u8(st))


# ---- 9. what the Python side refuses (nothing is launched) -----------------------------------------------------------------------------------------------
def test_python_refusals():
    from lqer_amd import PagedKVCache, attention_flexible_paged

    dt, d, h, hk, w = torch.float16, 48, 4, 2, 20
    cache = PagedKVCache(8, 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=6, window=w)
    long_, short = cache.alloc(), cache.alloc()
    k, v = _kv(70, d, hk, dt, 6400)
    _grow(cache, long_, k, v, 8)
    cache.append([short], k[:, :, :18], v[:, :, :18])
    assert cache.pt.released[cache.pt.slot(long_)] == 2
    q = _q(d, h, dt, 1, 2)
    snap = cache.buf.clone()
    with pytest.raises(ValueError, match="causal"):   # the cache's window is the default, and a window needs the causal rule
        attention_flexible_paged(q, cache, [long_], 1.0)
    with pytest.raises(ValueError, match="causal"):
        attention_flexible_paged(q, cache, [short], 1.0, window=5)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            attention_flexible_paged(q, cache, [long_], 1.0, causal=True, window=bad)
    with pytest.raises(ValueError, match="released"):  # wider than the cache's: those keys are gone
        attention_flexible_paged(q, cache, [long_], 1.0, causal=True, window=w + 1)
    q12 = _q(d, h, dt, 1, 12)
    for kernel in ("prefill", "auto"):
        with pytest.raises(ValueError, match="prefill"):  # beyond W keys the prefill kernel has no rule
            attention_flexible_paged(q12, cache, [long_], 1.0, causal=True, kernel=kernel)
    with pytest.raises(ValueError, match="released"):
        cache.to_dense(long_)
    with pytest.raises(ValueError, match="released"):
        cache.dequantized(long_)
    torch.cuda.synchronize()
    assert torch.equal(cache.buf, snap)
    # up to W keys the rule is a no-op: the prefill kernel runs as ever, and gives the bits of the unwindowed call on the raw tensors
    from lqer_amd import attention_flexible

    for kernel in ("prefill", "auto"):
        got, got_st = attention_flexible_paged(q12, cache, [short], d ** -0.5, causal=True, kernel=kernel, return_stats=True)
        want, want_st = attention_flexible(q12, k[:, :, :18], v[:, :, :18], CFG, CFG, d ** -0.5, causal=True, kernel="prefill", return_stats=True)
        assert torch.equal(u8(got), u8(want)) and torch.equal(u8(got_st), u8(want_st))
    assert cache.to_dense(short).length == 18  # nothing released: the export still works

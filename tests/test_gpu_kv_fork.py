"""Sequences over shared pages of the paged KV pool on the GPU (lqer_kv_pool_fork: k_kv_pool_fork in csrc/kv_cache.hip;
lqer_amd.kvcache.PagedKVCache.fork / fork_many / reorder) and the dense cache's batch gather (QuantizedKVCache.select, the cache
layer's reorder_cache for generate(num_beams=...)).

The contract is the paged pool's: a sequence gives the bits of the decode (or prefill) kernel on ITS raw K and V alone
(attention_flexible with batch 1 - never the paged code itself), and its bytes are those of a sequence that was appended the same
keys without any fork.  A forked sequence is no exception, whatever its parent and its siblings did afterwards.  Every comparison is
torch.equal on the bytes; there is no tolerance in this file.

Shapes: heads 4, kv heads 2; d 48 in the three dtypes, d 16 and d 128 in fp16.  Fork lengths 1, 15, 16, 17, 37, 261: inside the first
page, one key before / at / one key after a page boundary, two full pages and an open one, and 16 full pages (more than one chunk of
the decode kernel)."""
import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
import test_gpu_kv_paged as P

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES, DT_ID = F.CFG, F.DEV, F.DTYPES, P.DT_ID
H, HK = 4, 2
pages_of, u8 = P.pages_of, P.u8
FORMS = [(dt, 48) for dt in DTYPES] + [(torch.float16, 16), (torch.float16, 128)]
FORM_IDS = [f"{DT_ID[dt]}-d{d}" for dt, d in FORMS]


def _raw(n, d, dtype, seed):
    """Raw K and V [1, HK, n, d] on the device."""
    return tuple(x.to(DEV) for x in KV._kv((1, HK, n, d), dtype, seed, 2.0))


def _pool(pages, seqs, d, dtype, per_seq=None):
    from lqer_amd import PagedKVCache

    return PagedKVCache(pages, seqs, HK, d, CFG, CFG, dtype, DEV, max_pages_per_seq=per_seq or pages)


def _feed(cache, seqs, raws, patterns, at):
    """Append raws[i][at[i]:] to seqs[i] in pieces of patterns[i], one call per round over the sequences that still have a piece of
    that size - the calls of a decode batch where the pieces are single keys."""
    at, left = list(at), [list(p) for p in patterns]
    while any(left):
        n = next(p[0] for p in left if p)
        live = [i for i, p in enumerate(left) if p and p[0] == n]
        cache.append([seqs[i] for i in live], torch.cat([raws[i][0][:, :, at[i]:at[i] + n] for i in live]),
                     torch.cat([raws[i][1][:, :, at[i]:at[i] + n] for i in live]))
        for i in live:
            at[i] += n
            left[i].pop(0)
    assert at == [r[0].shape[2] for r in raws]


def _check_prefill(cache, seqs, raws, q):
    """kernel="prefill" over the pool against the prefill kernel on every sequence's raw K and V."""
    from lqer_amd import attention_flexible, attention_flexible_paged

    d = q.shape[3]
    out, st = attention_flexible_paged(q, cache, seqs, d ** -0.5, kernel="prefill", return_stats=True)
    for b, (k, v) in enumerate(raws):
        want, want_st = attention_flexible(q[b:b + 1], k, v, CFG, CFG, d ** -0.5, kernel="prefill", return_stats=True)
        assert torch.equal(u8(out[b:b + 1]), u8(want)) and torch.equal(u8(st[b:b + 1]), u8(want_st)), f"prefill: sequence {b} ({k.shape[2]} keys) differs"


def _check_attention(cache, seqs, raws, dtype, d, seed, what=""):
    """One paged call over `seqs` per form - decode s = 1, decode s = 3 causal, prefill s = 9 - against the raw tensors."""
    q = lambda s: F._randn((len(seqs), H, s, d), dtype, seed + s, 3.0).to(DEV)
    P._check_bits(cache, seqs, raws, q(1), False, what=what)
    if min(r[0].shape[2] for r in raws) >= 3:
        P._check_bits(cache, seqs, raws, q(3), True, what=what)
    _check_prefill(cache, seqs, raws, q(9))


def _check_twin(cache, seq, twin_cache, twin_seq, what):
    """The stored values and the live bytes of a sequence against a never-forked one with the same keys."""
    t = cache.length(seq)
    assert t == twin_cache.length(twin_seq)
    got, want = cache.dequantized(seq), twin_cache.dequantized(twin_seq)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{what}: dequantized values differ"
    P._same_live_bytes(cache.to_dense(seq), twin_cache.to_dense(twin_seq), t, what)


def _tails(lp):
    """Append patterns after a fork at lp for [parent, child, child]: single keys up to 13, 14, 15 keys in the open block (at least
    one), then one append of 5 keys - which so crosses a page boundary - and two more single keys."""
    return [[1] * (((13 + i - lp) % 16) or 16) + [5, 1, 1] for i in range(3)]


# ---- 1. bits after divergence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", [1, 15, 16, 17, 37, 261])
@pytest.mark.parametrize("dtype, d", FORMS, ids=FORM_IDS)
def test_bits_after_divergence(dtype, d, lp):
    pats = _tails(lp)
    prefix = _raw(lp, d, dtype, 5000 + lp)
    raws = []
    for i, p in enumerate(pats):  # the same first lp keys, then everyone's own
        k, v = _raw(sum(p), d, dtype, 5100 + 3 * lp + i)
        raws.append((torch.cat([prefix[0], k], 2), torch.cat([prefix[1], v], 2)))
    room = pages_of(lp + 40)
    cache, twin = _pool(3 * room, 3, d, dtype, room), _pool(3 * room, 3, d, dtype, room)
    parent = cache.alloc()
    cache.append([parent], *prefix)
    kids = cache.fork(parent, 2)
    assert len(kids) == 2 and len({parent, *kids}) == 3 and all(cache.length(s) == lp for s in kids)
    assert cache.pages_shared == lp // 16 and cache.pages_free == 3 * room - pages_of(lp) - 2 * (lp % 16 != 0)
    seqs = [parent, *kids]
    _feed(cache, seqs, raws, pats, [lp] * 3)
    tw = [twin.alloc() for _ in range(3)]
    _feed(twin, tw, raws, [[lp] + p for p in pats], [0] * 3)
    assert twin.pages_shared == 0 and cache.pages_shared == lp // 16
    assert cache.pages_free - twin.pages_free == 2 * (lp // 16)  # what sharing saves: the full pages, twice
    _check_attention(cache, seqs, raws, dtype, d, 50, what=f"fork at {lp}:")
    for s, t, name in zip(seqs, tw, ("parent", "child 0", "child 1")):
        _check_twin(cache, s, twin, t, f"fork at {lp}, {name}")


# ---- 2. the launch touches only what it owns -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", [5, 37, 16, 32])
@pytest.mark.parametrize("dtype, d", [(torch.float16, 48), (torch.float32, 16), (torch.bfloat16, 128)], ids=["f16-d48", "f32-d16", "bf16-d128"])
def test_fork_writes_the_children_tail_items_and_staging_rows_only(dtype, d, lp):
    """Children on dirty pages and dirty slots (an earlier sequence's, overwritten with 0xFF), pool and table between guard zones."""
    stride = 4
    cache = _pool(10, 3, d, dtype, stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=1, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(3, stride)
    junk = [cache.alloc(), cache.alloc()]
    for i, s in enumerate(junk):
        cache.append([s], *_raw(40, d, dtype, 6000 + i))
    parent = cache.alloc()
    k, v = _raw(lp + 24, d, dtype, 6010 + lp)
    cache.append([parent], k[:, :, :lp], v[:, :, :lp])
    junk_slots = [cache.pt.slot(s) for s in junk]
    junk_pages = [p for s in junk_slots for p in cache.pt.table[s][:3]]
    for s in junk:
        cache.free(s)
    for slot in junk_slots:
        for lo, hi in P._pool_spans(cache, junk_pages, slot):
            cache.buf[lo:hi].fill_(0xFF)
    torch.cuda.synchronize()
    snap, free0 = g_pool.payload.clone(), cache.pages_free
    kids = cache.fork(parent, 2)
    torch.cuda.synchronize()
    g_pool.check(), g_tbl.check()
    slots = [cache.pt.slot(s) for s in kids]
    assert sorted(slots) == sorted(junk_slots)
    tails = [cache.pt.table[s][lp // 16] for s in slots] if lp % 16 else []
    assert set(tails) <= set(junk_pages) and len(set(tails)) == len(tails) and cache.pages_free == free0 - len(tails)
    allowed = torch.zeros(snap.numel(), dtype=torch.bool, device=DEV)
    staging = torch.zeros_like(allowed)
    for i, slot in enumerate(slots):
        spans = P._pool_spans(cache, tails[i:i + 1], slot)
        for lo, hi in spans:
            allowed[lo:hi] = True
        staging[spans[-1][0]:spans[-1][1]] = True
    changed = g_pool.payload != snap
    assert not bool((changed & ~allowed).any()), f"{int((changed & ~allowed).sum())} bytes changed outside the children's tail pages {tails} and staging rows"
    assert bool(changed.any())  # (the dirt is gone from the staging rows at least)
    if lp % 16 == 0:
        assert not bool((changed & ~staging).any()), "a full parent: no code or exponent byte may change"
    # the parent is as it was, and the children - on the dirty pages and slots - go on with the bits
    pats = [[1, 5, 1], [5, 1, 1, 1], [1] * 8]
    raws = []
    for i, p in enumerate(pats):
        kn, vn = _raw(sum(p), d, dtype, 6100 + lp + i)
        raws.append((torch.cat([k[:, :, :lp], kn], 2), torch.cat([v[:, :, :lp], vn], 2)))
    _feed(cache, [parent, *kids], raws, pats, [lp] * 3)
    torch.cuda.synchronize()
    g_pool.check(), g_tbl.check()
    _check_attention(cache, [parent, *kids], raws, dtype, d, 60, what=f"dirty pages, fork at {lp}:")


# ---- 3. lifetime ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", [37, 32, 5])
def test_lifetime_of_shared_pages(lp):
    dtype, d, n, num = torch.float16, 48, 2, 14
    cache = _pool(num, 4, d, dtype, 4)
    k, v = _raw(lp, d, dtype, 7000 + lp)
    parent = cache.alloc()
    cache.append([parent], k, v)
    kids = cache.fork(parent, n)
    tail = int(lp % 16 != 0)
    assert cache.pages_free == num - (pages_of(lp) + n * tail) and cache.pages_shared == lp // 16
    cache.free(parent)  # right after the fork: the children keep the full pages
    assert cache.pages_free == num - (lp // 16 + n * tail) and cache.pages_shared == lp // 16
    _check_attention(cache, kids, [(k, v)] * 2, dtype, d, 70, what="parent freed:")
    # a fork of a fork, and everyone grows apart
    (grand,) = cache.fork(kids[1])
    assert cache.pages_free == num - (lp // 16 + 3 * tail) and cache.pages_shared == lp // 16
    seqs, pats = [*kids, grand], [[1, 1, 5], [5, 1], [1] * 12]
    raws = []
    for i, p in enumerate(pats):
        kn, vn = _raw(sum(p), d, dtype, 7100 + lp + i)
        raws.append((torch.cat([k, kn], 2), torch.cat([v, vn], 2)))
    _feed(cache, seqs, raws, pats, [lp] * 3)
    _check_attention(cache, seqs, raws, dtype, d, 71, what="fork of a fork:")
    twin = _pool(num, 4, d, dtype, 4)
    for s, raw in zip(seqs, raws):
        t = twin.alloc()
        twin.append([t], *raw)
        _check_twin(cache, s, twin, t, f"sequence {s}")
        twin.free(t)
    cache.free(kids[0])
    assert cache.pages_shared == lp // 16  # two owners left
    cache.free(grand)
    assert cache.pages_shared == 0 and cache.pages_free == num - pages_of(cache.length(kids[1]))
    cache.free(kids[1])
    assert cache.pages_free == num == cache.num_pages and sorted(cache.pt._free_pages) == list(range(num))
    fresh, raw = cache.alloc(), _raw(61, d, dtype, 7200)
    cache.append([fresh], *raw)  # on the pages everyone gave back
    _check_attention(cache, [fresh], [raw], dtype, d, 72, what="reused pages:")


def test_fork_many_parents_and_empty_parents():
    """One call, several parents, repeats; a parent of length 0 gives empty children and launches nothing."""
    dtype, d = torch.bfloat16, 48
    cache = _pool(12, 7, d, dtype, 3)
    lens = (21, 16)
    raws = [_raw(n + 3, d, dtype, 7300 + n) for n in lens]
    a, b, e = cache.alloc(), cache.alloc(), cache.alloc()
    for s, (k, v), n in zip((a, b), raws, lens):
        cache.append([s], k[:, :, :n], v[:, :, :n])
    snap = cache.buf.clone()
    assert cache.fork(e, 1) and torch.equal(cache.buf, snap)  # empty parent, empty child, no byte moved
    kids = cache.fork_many([b, a, b])
    assert [cache.length(s) for s in kids] == [16, 21, 16] and cache.pages_shared == 2 and cache.pages_free == 12 - 3 - 1
    with pytest.raises(RuntimeError):
        cache.fork(a)  # no slot left
    with pytest.raises(KeyError):
        cache.fork(99)
    seqs, rr = [a, b, *kids], [raws[0], raws[1], raws[1], raws[0], raws[1]]
    _feed(cache, seqs, rr, [[3]] * 5, [21, 16, 16, 21, 16])
    _check_attention(cache, seqs, rr, dtype, d, 73)


# ---- 4. beam steps -------------------------------------------------------------------------------------------------------------------
def test_beam_steps():
    """Width 3, prompts of 14 keys, four steps of one key per beam - lengths 15, 16, 17, 18: a step forks inside the first page, one at
    the page boundary, one behind it."""
    dtype, d, num = torch.float16, 48, 9
    cache = _pool(num, 4, d, dtype, 3)
    beams = [cache.alloc() for _ in range(3)]
    hist = [_raw(14, d, dtype, 8000 + i) for i in range(3)]
    for s, (k, v) in zip(beams, hist):
        cache.append([s], k, v)
    for step, idx in enumerate([[0, 0, 0], [2, 0, 1], [1, 1, 2], [2, 2, 0]]):
        free0, snap = cache.pages_free, cache.buf.clone()
        new = cache.reorder(beams, idx)
        assert len(new) == 3 and len(set(new)) == 3
        if sorted(idx) == [0, 1, 2]:  # a permutation: the ids move, nothing else does
            assert new == [beams[j] for j in idx] and cache.pages_free == free0 and torch.equal(cache.buf, snap)
        else:
            assert all(new[idx.index(j)] == beams[j] for j in set(idx))  # the first to continue a parent keeps its id
            assert all(new[i] not in beams for i, j in enumerate(idx) if idx.index(j) != i)  # the others are new sequences
            gone = [s for j, s in enumerate(beams) if j not in idx]
            for s in gone:
                with pytest.raises(KeyError):
                    cache.length(s)
        beams, hist = new, [hist[j] for j in idx]
        kn, vn = _raw(3, d, dtype, 8100 + step)  # [1, HK, 3, d]: one new key per beam
        kn, vn = kn[0].transpose(0, 1)[:, :, None], vn[0].transpose(0, 1)[:, :, None]
        cache.append(beams, kn.contiguous(), vn.contiguous())
        hist = [(torch.cat([k, kn[i:i + 1]], 2), torch.cat([v, vn[i:i + 1]], 2)) for i, (k, v) in enumerate(hist)]
        assert [cache.length(s) for s in beams] == [15 + step] * 3
        _check_attention(cache, beams, hist, dtype, d, 80 + step, what=f"beam step {step} {idx}:")
        for s, (k, v) in zip(beams, hist):  # the twin: rebuilt from the beam's own raw history
            twin = KV._cache(k, v, capacity=cache.to_dense(s).capacity)
            got, want = cache.dequantized(s), twin.dequantized()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            P._same_live_bytes(cache.to_dense(s), twin, k.shape[2], f"beam step {step}, sequence {s}")
    live = {p for s in beams for p in cache.pt.table[cache.pt.slot(s)][:2]}
    assert cache.pages_free == num - len(live)


def test_a_reorder_the_pool_cannot_serve_changes_nothing():
    dtype, d = torch.float16, 48
    cache = _pool(3, 3, d, dtype, 2)
    a, b, c = (cache.alloc() for _ in range(3))
    raws = [_raw(5, d, dtype, 8200 + i) for i in range(3)]
    for s, (k, v) in zip((a, b, c), raws):
        cache.append([s], k, v)
    state = lambda: (cache.pages_free, [r[:] for r in cache.pt.table], cache.pt.lengths[:], cache.pt.pages_of[:], dict(cache.pt._slot))
    before, snap, tbl = state(), cache.buf.clone(), cache.table.clone()
    with pytest.raises(RuntimeError):
        cache.reorder([a, b], [0, 0, 0])  # b's page and slot serve one fork; the second has no page (c lives on)
    with pytest.raises(ValueError):
        cache.reorder([a, b], [0, 2])
    with pytest.raises(ValueError):
        cache.reorder([a, a], [0, 1])
    with pytest.raises(KeyError):
        cache.reorder([a, 7], [0, 0])
    assert state() == before and torch.equal(cache.buf, snap) and torch.equal(cache.table, tbl)
    _check_attention(cache, [a, b, c], raws, dtype, d, 82)
    new = cache.reorder([a, b, c], [1, 1, 1])  # a's and c's pages serve the forks
    assert new[0] == b and cache.pages_free == 0
    _check_attention(cache, new, [raws[1]] * 3, dtype, d, 83)


# ---- 5. taking speculated tokens back --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", [14, 37, 32])
def test_speculation_rollback_recipe(lp):
    dtype, d = torch.float16, 48
    cache, twin = _pool(8, 2, d, dtype, 4), _pool(8, 2, d, dtype, 4)
    k, v = _raw(lp + 5, d, dtype, 9000 + lp)
    seq = cache.alloc()
    cache.append([seq], k[:, :, :lp], v[:, :, :lp])
    snap, = cache.fork(seq)
    cache.append([seq], k[:, :, lp:], v[:, :, lp:])  # the speculated block
    _check_attention(cache, [seq], [(k, v)], dtype, d, 90)
    cache.free(seq)  # two of the five are accepted
    cache.append([snap], k[:, :, lp:lp + 2], v[:, :, lp:lp + 2])
    kept = (k[:, :, :lp + 2], v[:, :, :lp + 2])
    t = twin.alloc()
    twin.append([t], kept[0][:, :, :lp], kept[1][:, :, :lp])
    twin.append([t], kept[0][:, :, lp:], kept[1][:, :, lp:])
    _check_attention(cache, [snap], [kept], dtype, d, 91, what="after the rollback:")
    _check_twin(cache, snap, twin, t, f"rolled back to {lp + 2}")
    assert cache.pages_free == twin.pages_free and cache.pages_shared == 0


# ---- 6. the dense cache: select ----------------------------------------------------------------------------------------------------------
def _same_live_bytes_batch(cache, ref, what):
    """P._same_live_bytes for any batch: the live part of the five sections of two dense caches of one shape."""
    from lqer_amd.kvcache import _sections

    assert (cache.batch, cache.capacity, cache.length) == (ref.batch, ref.capacity, ref.length) and cache.buf.numel() == ref.buf.numel()
    t, hk, d, z = cache.length, cache.kv_heads, cache.head_dim, cache.batch * cache.kv_heads
    esz = torch.empty((), dtype=cache.dtype).element_size()
    secs, total = _sections(cache.dtype, cache.batch, hk, cache.capacity, d)
    assert total == cache.buf.numel()
    blocks, full = pages_of(t), t // 16
    for name, at, per_block in secs:
        row = 16 * d * esz if per_block is None else (cache.capacity // 16) * per_block
        live = torch.zeros(row, dtype=torch.bool, device=DEV)
        if name == "k_stage":
            live[:(t % 16) * d * esz] = True
        elif name in ("k_codes", "k_exps"):
            live[:blocks * per_block] = True
        elif name == "v_codes":
            live[:t * d] = True
        else:
            live[:full * per_block] = True
            if t % 16:
                live[full * per_block:blocks * per_block].view(d // 16, 16)[:, :t % 16] = True
        a, r = (x.buf[at:at + z * row].view(z, row)[:, live] for x in (cache, ref))
        assert torch.equal(a, r), f"{what}: section {name} differs in {(a != r).sum().item()} of {a.numel()} live bytes"


@pytest.mark.parametrize("t", [21, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
def test_dense_select(dtype, t):
    from lqer_amd import attention_flexible_cached

    d, idx = 48, [2, 0, 0, 1]
    k, v = (x.to(DEV) for x in KV._kv((3, HK, t + 2, d), dtype, 9100 + t, 2.0))
    cache = KV._cache(k[:, :, :t], v[:, :, :t], capacity=64)
    cache.select(idx)
    want = KV._cache(k[idx][:, :, :t], v[idx][:, :, :t], capacity=64)
    assert cache.batch == 4 and cache.length == t and cache.capacity == 64
    _same_live_bytes_batch(cache, want, f"select at {t}")
    for step in range(3):  # as it is, then after one and two more keys: the staging rows moved with the rows
        for s, causal in ((1, False), (3, True)):
            q = F._randn((4, H, s, d), dtype, 95 + s + step, 3.0).to(DEV)
            got, want_o = (attention_flexible_cached(q, c, d ** -0.5, causal=causal, return_stats=True) for c in (cache, want))
            assert torch.equal(u8(got[0]), u8(want_o[0])) and torch.equal(u8(got[1]), u8(want_o[1])), f"select at {t}, {step} keys later, s = {s}"
        if step < 2:
            cache.append(k[idx][:, :, t + step:t + step + 1], v[idx][:, :, t + step:t + step + 1])
            want.append(k[idx][:, :, t + step:t + step + 1], v[idx][:, :, t + step:t + step + 1])
            _same_live_bytes_batch(cache, want, f"select at {t}, {step + 1} keys later")
    cache.select(torch.tensor([3, 1], device=DEV))  # a tensor, and a smaller batch
    assert cache.batch == 2
    _same_live_bytes_batch(cache, KV._cache(k[[1, 0]], v[[1, 0]], capacity=64), "select to a smaller batch")
    for bad in ([], [2], [-1, 0]):
        with pytest.raises(ValueError):
            cache.select(bad)
    assert cache.batch == 2 and cache.length == t + 2


def test_generate_with_beams():
    """generate(num_beams=3) over the packed cache returns the sequences of the same call over a DynamicCache: transformers' beam search
    reorders the cache through Cache.reorder_cache at every step, which the layers route to QuantizedKVCache.select."""
    from transformers import DynamicCache

    model, qc, A = KV._model("llama-gqa")
    model = A.enable_quantized_attention(model, qc, fused=True).to(DEV)
    ids = torch.randint(0, 200, (2, 20), generator=torch.Generator().manual_seed(13)).to(DEV)
    cls, calls = A._kv_layer_cls(), []
    real = cls.reorder_cache

    def counted(self, beam_idx):
        calls.append(beam_idx.tolist())
        return real(self, beam_idx)

    cls.reorder_cache = counted
    try:
        packed = A.quantized_kv_cache(model)
        kw = dict(num_beams=3, max_new_tokens=20, do_sample=False, pad_token_id=0, attention_mask=torch.ones_like(ids))
        with torch.no_grad():
            got = model.generate(ids, past_key_values=packed, **kw)
            n_calls = len(calls)
            want = model.generate(ids, past_key_values=DynamicCache(), **kw)
    finally:
        cls.reorder_cache = real
    assert n_calls >= model.config.num_hidden_layers and len(calls) == n_calls  # the packed run went through reorder_cache, the other did not
    assert any(c != sorted(c) or len(set(c)) < len(c) for c in calls), "no step reordered anything: the test shows nothing"
    assert got.shape == want.shape and torch.equal(got, want)
    assert packed.layers[0].cache.batch == 6

    # the two other batch operations of a cache layer
    layer = packed.layers[0]
    before = layer.cache.dequantized()
    layer.batch_select_indices(torch.tensor([4, 1], device=DEV))
    after = layer.cache.dequantized()
    assert layer.cache.batch == 2 and torch.equal(after[0], before[0][[4, 1]]) and torch.equal(after[1], before[1][[4, 1]])
    layer.batch_repeat_interleave(3)
    rep = layer.cache.dequantized()
    assert layer.cache.batch == 6 and torch.equal(rep[0], after[0].repeat_interleave(3, 0)) and torch.equal(rep[1], after[1].repeat_interleave(3, 0))
    for fn in (layer.crop, layer.offload):
        with pytest.raises(NotImplementedError):
            fn()

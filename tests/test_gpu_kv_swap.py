"""Copying pages between paged KV pools and swapping sequences out and in on the GPU (lqer_kv_pool_copy: k_kv_pool_copy in
csrc/kv_cache.hip; lqer_amd.kvcache.PagedKVCache.export / adopt / swap_out / swap_in / adopt_from, KVPoolImage).

The guarantee under test: an adopted sequence is a sequence like any other - the attention entries, later appends, fork and to_dense give
on it the SAME BITS as on the sequence it was exported from, whatever pages it lands on, whichever pool it lands in, whether or not the
image went through the host or a file.  Bytes move as they are, so nothing here has a tolerance: every comparison is torch.equal.  All
pools start as 0xFF and the destination's free stack is scrambled, so a page that did not travel, or travelled to the wrong place, shows.

Shapes: kv heads 2, heads 4; bf16 at d = 64 (the base), d = 16 and d = 128 (272 pieces of 16 bytes per item: the second round of the
copy loop), fp32 once (the largest staging rows), nibble codes (4, 4) and (8, 4) at d = 128.  Sequences of 0, 5, 16 and 37 keys (none,
an open block, a full page and no open block, two pages and an open block) and a parent of 40 keys forked twice, the children grown
by 3 and 21 keys."""
import pytest
import torch

import _attention as A
import _formats as F
import test_gpu_kv_paged as P

pytestmark = pytest.mark.gpu

DEV = A.DEV
H, HK = 4, 2
_X, _W = F.cfg("e8", 8, [1, 16], True), F.cfg("e8", 4, [1, 16], True)
CFG = dict(name="flexible", default=_X, x_quantizer=_X, w_quantizer=_W)  # K and V of width 4: byte and nibble pools take it
FORMS = [(torch.bfloat16, 64, None), (torch.bfloat16, 16, None), (torch.bfloat16, 128, None), (torch.float32, 64, None),
         (torch.bfloat16, 128, (4, 4)), (torch.bfloat16, 128, (8, 4))]
FORM_IDS = ["bf16-d64", "bf16-d16", "bf16-d128", "f32-d64", "bf16-d128-K4V4", "bf16-d128-K8V4"]
BASE = FORMS[0]
LENS = (0, 5, 16, 37)
ALL_LENS = LENS + (40, 43, 61)
u8 = lambda t: t.contiguous().view(torch.uint8)


def kv(n, d, dtype, seed, batch=1):
    """Raw K and V [batch, HK, n, d] on the device."""
    return A._randn((batch, HK, n, d), dtype, seed).to(DEV), A._randn((batch, HK, n, d), dtype, seed + 1).to(DEV)


def make(dtype, d, bits=None, pages=24, slots=10, room=6, **kw):
    from lqer_amd import PagedKVCache

    cache = PagedKVCache(pages, slots, HK, d, CFG, CFG, dtype, DEV, max_pages_per_seq=room, code_bits=bits, **kw)
    cache.buf.fill_(0xFF)
    return cache


def source(dtype, d, bits=None):
    """The fixture's pool: sequences of LENS keys, a parent of 40 keys forked twice, the children grown apart - ALL_LENS in all."""
    cache = make(dtype, d, bits)
    seqs = []
    for n in LENS:
        seqs.append(cache.alloc())
        if n:
            cache.append([seqs[-1]], *kv(n, d, dtype, 100 + n))
    parent = cache.alloc()
    cache.append([parent], *kv(40, d, dtype, 200))
    kids = cache.fork(parent, 2)
    cache.append([kids[0]], *kv(3, d, dtype, 210))
    cache.append([kids[1]], *kv(21, d, dtype, 220))
    seqs += [parent, *kids]
    assert tuple(cache.length(s) for s in seqs) == ALL_LENS and cache.pages_shared == 2 and cache.pages_free == 24 - 11
    return cache, seqs


def scrambled(dtype, d, bits=None, **kw):
    """A destination pool whose free stack no longer counts up: sequences were appended and freed out of order, and two stay live.
    Its freed pages hold those sequences' bytes, not 0xFF."""
    cache = make(dtype, d, bits, pages=40, slots=12, **kw)
    junk = []
    for i, n in enumerate((33, 17, 50, 90)):
        junk.append(cache.alloc())
        for at in range(0, n, 30):  # (pieces a windowed pool takes too)
            cache.append([junk[-1]], *kv(min(30, n - at), d, dtype, 300 + 10 * i + at))
    cache.free(junk[0]), cache.free(junk[2])
    return cache


def held(cache, seq):
    s = cache.pt.slot(seq)
    return cache.pt.table[s][cache.pt.released[s]:cache.pt.pages_of[s]]


def books(cache):
    pt = cache.pt
    return (pt.pages_free, pt.pages_shared, [row[:] for row in pt.table], pt.pages_of[:], pt.lengths[:], pt.released[:], pt._free_pages[:],
            pt._free_slots[:], dict(pt._slot), pt._next_seq, pt._owners.tolist())


def dense_blocks(cache, seq):
    """to_dense(seq): every block of 16 keys up to the length, whole, in the four code and exponent sections, and the staging rows, whole
    - what travels; the sections' padding, which nothing writes, left out."""
    from lqer_amd.kvcache import _sections

    dense = cache.to_dense(seq)
    secs, _ = _sections(dense.dtype, 1, HK, dense.capacity, dense.head_dim)
    esz = torch.empty((), dtype=dense.dtype).element_size()
    out = []
    for _, at, per_block in secs:
        size = HK * (16 * dense.head_dim * esz if per_block is None else (dense.capacity // 16) * per_block)
        out.append(dense.buf[at:at + size])
    return torch.cat(out)


def outputs(cache, seqs, seed=0):
    """One paged call per form - decode s = 1, decode s = 8, prefill s = 12, causal - over the sequences that hold at least s keys: every
    out and row_stats.  The queries depend on (seed, s, position in `seqs`) alone."""
    from lqer_amd import attention_flexible_paged

    lens, d, res = [cache.length(s) for s in seqs], cache.head_dim, []
    for s, kernel in ((1, "decode"), (8, "decode"), (12, "prefill")):
        idx = [i for i, n in enumerate(lens) if n >= s]
        q = A._randn((len(seqs), H, s, d), cache.dtype, 900 + 17 * seed + s).to(DEV)[idx]
        res += attention_flexible_paged(q, cache, [seqs[i] for i in idx], d ** -0.5, causal=True, return_stats=True, kernel=kernel)
    return res


def same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(u8(a), u8(b)), f"{what}: item {i}: {(u8(a) != u8(b)).sum().item()} of {u8(a).numel()} bytes differ"


def same_live(cache, seqs, ref, ref_seqs, what):
    for a, b in zip(seqs, ref_seqs):
        t = cache.length(a)
        assert t == ref.length(b)
        if t:
            P._same_live_bytes(cache.to_dense(a), ref.to_dense(b), t, f"{what}: sequence of {t} keys")


# ---- 1. the same bits after a swap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", ["host", "file"])
@pytest.mark.parametrize("dtype, d, bits", FORMS, ids=FORM_IDS)
def test_same_bits_after_swap(dtype, d, bits, via, tmp_path):
    from lqer_amd import KVPoolImage

    src, seqs = source(dtype, d, bits)
    want = outputs(src, seqs) + [dense_blocks(src, s) for s, n in zip(seqs, ALL_LENS) if n]
    shared, src_pages = src.pages_shared, [held(src, s) for s in seqs]
    image = src.swap_out(seqs)
    assert src.pages_free == 24 and src.pt._slot == {}  # preempted: everything is back in the pool
    assert not image.buf.is_cuda and image.buf.is_pinned() and image.pages == 11 and image.slots == 7 and image.lengths == list(ALL_LENS)
    assert image.nbytes == image.buf.numel() < src.nbytes
    with pytest.raises(KeyError):
        src.length(seqs[1])
    if via == "file":
        torch.save(image.state_dict(), tmp_path / "image.pt")
        image = KVPoolImage.from_state_dict(torch.load(tmp_path / "image.pt"))
        assert image.ready is None and image.pages == 11 and image.lengths == list(ALL_LENS)
    dst = scrambled(dtype, d, bits)
    new = dst.swap_in(image)
    assert len(new) == 7 and [dst.length(s) for s in new] == list(ALL_LENS) and dst.pages_shared == shared == 2
    for a, b in zip((p for s in new for p in held(dst, s)), (p for row in src_pages for p in row)):
        assert a != b  # no page id survived
    assert [len(held(dst, s)) for s in new] == [len(r) for r in src_pages]
    same(outputs(dst, new) + [dense_blocks(dst, s) for s, n in zip(new, ALL_LENS) if n], want, f"after swap_in ({via})")
    # ... and back into the pool it left, on whatever pages are free there now
    other = src.alloc()
    src.append([other], *kv(50, d, dtype, 400))
    back = src.adopt(image)
    assert src.pages_shared == 2
    same(outputs(src, back) + [dense_blocks(src, s) for s, n in zip(back, ALL_LENS) if n], want, f"back in the first pool ({via})")


# ---- 2. later appends: the staging rows travelled ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [None, "cpu"], ids=["device-image", "host-image"])
@pytest.mark.parametrize("dtype, d, bits", FORMS, ids=FORM_IDS)
def test_later_appends_give_the_same_bits(dtype, d, bits, device):
    from lqer_amd import attention_flexible_paged

    src, seqs = source(dtype, d, bits)
    before = books(src)
    image = src.export(seqs, device=device)
    assert books(src) == before and image.buf.is_cuda == (device is None)  # the originals stay live
    dst = scrambled(dtype, d, bits)
    new = dst.adopt(image)
    k, v = kv(20, d, dtype, 500, batch=7)
    src.append(seqs, k, v)  # 5 + 20 and 37 + 20: the open blocks' raw keys are re-quantized with the new ones; 16 + 20: none were open
    dst.append(new, k, v)
    assert [dst.length(s) for s in new] == [n + 20 for n in ALL_LENS]
    same(outputs(dst, new, 1), outputs(src, seqs, 1), "after 20 more keys")
    same_live(dst, new, src, seqs, "after 20 more keys")
    # counts of their own, a fork of a copy, and the copy's fork against the original's
    counts = [3, 0, 16, 1, 7, 0, 2]
    kr, vr = (x[0].transpose(0, 1).contiguous() for x in kv(sum(counts), d, dtype, 510))
    src.append_ragged(seqs, kr, vr, counts), dst.append_ragged(new, kr, vr, counts)
    (fa,), (fb,) = src.fork(seqs[3]), dst.fork(new[3])
    k1, v1 = kv(5, d, dtype, 520)
    src.append([fa], k1, v1), dst.append([fb], k1, v1)
    same(outputs(dst, new + [fb], 2), outputs(src, seqs + [fa], 2), "after a ragged append and a fork")
    same_live(dst, new + [fb], src, seqs + [fa], "after a ragged append and a fork")
    q = A._randn((8, H, 1, d), dtype, 530).to(DEV)
    a, b = (attention_flexible_paged(q, c, s, d ** -0.5, shared_prefix=True) for c, s in ((dst, new + [fb]), (src, seqs + [fa])))
    same([a], [b], "shared_prefix over the copies")


# ---- 3. the window ---------------------------------------------------------------------------------------------------------------------------
def test_window_released_pages_travel_as_released():
    from lqer_amd import attention_flexible_paged

    dtype, d, _ = BASE
    cache = make(dtype, d, pages=30, slots=6, room=9, window=32, max_query_rows=16)
    seq = cache.alloc()
    for at in range(0, 100, 25):
        cache.append([seq], *kv(25, d, dtype, 600 + at))
    gone = cache.pt.released[cache.pt.slot(seq)]
    assert cache.length(seq) == 100 and gone >= 2 and cache.pages_held(seq) == 7 - gone
    with pytest.raises(ValueError):
        cache.to_dense(seq)  # the route that existed refuses such a sequence
    image = cache.export([seq])
    assert image.pages == 7 - gone and image.books["seqs"][0][:2] == (100, gone)
    copy, = cache.adopt(image)  # into the same pool, on pages of its own
    via_host, = cache.swap_in(cache.export([seq], device="cpu"))
    assert cache.pt.released[cache.pt.slot(copy)] == gone and not set(held(cache, copy)) & set(held(cache, seq))
    for s, kernel in ((1, "decode"), (8, "decode"), (12, "prefill")):
        q = A._randn((1, H, s, d), dtype, 610 + s).to(DEV).expand(3, H, s, d).contiguous()
        out, st = attention_flexible_paged(q, cache, [seq, copy, via_host], d ** -0.5, causal=True, return_stats=True, kernel=kernel)
        same([out[1:2], st[1:2], out[2:3], st[2:3]], [out[0:1], st[0:1]] * 2, f"windowed {kernel} s={s}")
    k, v = kv(20, d, dtype, 620)
    cache.append([seq, copy, via_host], torch.cat([k] * 3), torch.cat([v] * 3))  # the window moves on, alike for all three
    assert len({cache.pt.released[cache.pt.slot(s)] for s in (seq, copy, via_host)}) == 1
    q = A._randn((1, H, 12, d), dtype, 630).to(DEV).expand(3, H, 12, d).contiguous()
    out = attention_flexible_paged(q, cache, [seq, copy, via_host], d ** -0.5, causal=True, kernel="prefill")
    same([out[1:2], out[2:3]], [out[0:1]] * 2, "windowed prefill after 20 more keys")
    # a cache without that window: the keys below are gone, and only that rule never reads them
    for kw in (dict(), dict(window=32), dict(window=48, max_query_rows=16), dict(window=32, max_query_rows=24)):
        plain = scrambled(dtype, d, **kw)
        before, pool = books(plain), plain.buf.clone()
        with pytest.raises(ValueError, match="window"):
            plain.adopt(image)
        with pytest.raises(ValueError, match="window"):
            plain.adopt_from(cache, [seq])
        assert books(plain) == before and torch.equal(plain.buf, pool)
    # ... while a sequence that has released nothing goes anywhere
    young = cache.alloc()
    cache.append([young], *kv(30, d, dtype, 640))
    plain = scrambled(dtype, d)
    got, = plain.adopt_from(cache, [young])
    assert plain.length(got) == 30
    # another dtype, head dim or storage is refused whatever was released
    for other in (scrambled(torch.float16, d), scrambled(dtype, 32), scrambled(dtype, d, (4, 4))):
        before = books(other)
        with pytest.raises(ValueError, match="geometry"):
            other.adopt(cache.export([young]))
        assert books(other) == before


# ---- 4. pool to pool, no image ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d, bits", [FORMS[0], FORMS[4]], ids=[FORM_IDS[0], FORM_IDS[4]])
def test_adopt_from_between_two_pools_and_within_one(dtype, d, bits):
    src, seqs = source(dtype, d, bits)
    want = outputs(src, seqs) + [dense_blocks(src, s) for s, n in zip(seqs, ALL_LENS) if n]
    before, pool = books(src), src.buf.clone()
    dst = scrambled(dtype, d, bits)
    new = dst.adopt_from(src, seqs)
    assert books(src) == before and torch.equal(src.buf, pool)  # the source is only read
    assert dst.pages_shared == 2 and [dst.length(s) for s in new] == list(ALL_LENS)
    same(outputs(dst, new) + [dense_blocks(dst, s) for s, n in zip(new, ALL_LENS) if n], want, "adopt_from another pool")
    # within one pool: the three sequences that share pages, onto pages of their own
    twins = src.adopt_from(src, seqs[4:])
    assert src.pages_shared == 4 and src.pages_free == 24 - 11 - 6
    assert not {p for s in twins for p in held(src, s)} & {p for s in seqs for p in held(src, s)}
    same(outputs(src, seqs) + [dense_blocks(src, s) for s, n in zip(seqs, ALL_LENS) if n], want, "the originals after adopt_from within the pool")
    same(outputs(src, seqs[:4] + twins) + [dense_blocks(src, s) for s, n in zip(seqs[:4] + twins, ALL_LENS) if n], want, "adopt_from within one pool")
    for bad, exc in (([seqs[0], seqs[0]], ValueError), ([99], KeyError), ([], ValueError)):
        before = books(dst)
        with pytest.raises(exc):
            dst.adopt_from(src, bad)
        assert books(dst) == before


# ---- 5. the image is a pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, d, bits", [FORMS[0], FORMS[4]], ids=[FORM_IDS[0], FORM_IDS[4]])
def test_the_device_image_is_a_pool_of_its_own(dtype, d, bits):
    """The image's buffer under a fresh cache of the image's page and slot counts, the books adopted by a fresh table - which hands out
    pages and slots 0, 1, 2, ...: identity rows -, and nothing copied: the attention entries read the image as they read a pool."""
    from lqer_amd.kvcache import pool_bytes

    src, seqs = source(dtype, d, bits)
    want = outputs(src, seqs)
    image = src.export(seqs)
    assert image.buf.is_cuda and image.pages == 11 and image.slots == 7
    view = make(dtype, d, bits, pages=image.pages, slots=image.slots)
    assert view.nbytes == image.nbytes == pool_bytes(dtype, 11, 7, HK, d, *view._code_fmts())
    view.buf = image.buf
    new, slots, pages = view.pt.adopt(image.books)
    assert pages == list(range(11)) and slots == list(range(7))
    view._upload_rows(slots, [1] * 7)
    same(outputs(view, new), want, "the image read as a pool")
    empty = src.export([seqs[0]])  # only an empty sequence: no page travels
    assert empty.books["pages"] == [] and empty.lengths == [0] and empty.nbytes == pool_bytes(dtype, 1, 1, HK, d, *view._code_fmts())
    got, = src.adopt(empty)
    assert src.length(got) == 0 and held(src, got) == []


# ---- 6. rollback -----------------------------------------------------------------------------------------------------------------------------
def test_an_adopt_the_pool_cannot_serve_leaves_it_untouched():
    dtype, d, bits = BASE
    src, seqs = source(dtype, d, bits)
    for image in (src.export(seqs), src.export(seqs, device="cpu")):
        for kw, what in ((dict(pages=10, slots=8), "pages"), (dict(pages=24, slots=6), "slots"), (dict(pages=24, slots=8, room=3), "max_pages_per_seq")):
            dst = make(dtype, d, bits, **kw)
            live = dst.alloc()
            dst.append([live], *kv(7, d, dtype, 700))
            before, pool, table = books(dst), dst.buf.clone(), dst.table.clone()
            with pytest.raises(RuntimeError, match="adopt"):
                dst.adopt(image)
            with pytest.raises(RuntimeError, match="adopt"):
                dst.adopt_from(src, seqs)
            torch.cuda.synchronize()
            assert books(dst) == before and torch.equal(dst.buf, pool) and torch.equal(dst.table, table), what
    # a refusal behind the reservation: the books go back, and the next adopt takes the same ids, slots and pages
    dst = scrambled(dtype, d, bits)
    before, pool = books(dst), dst.buf.clone()
    image = src.export(seqs)
    short = type(image)(image.buf[:-256], image.pages, image.books, image.signature, image.ready)
    with pytest.raises(ValueError, match="image"):
        dst.adopt(short)
    strip = lambda bk: bk[:2] + ([bk[2][s] for s in dst.pt._slot.values()],) + bk[3:]
    assert strip(books(dst)) == strip(before) and torch.equal(dst.buf, pool)
    new = dst.adopt(image)
    assert new == list(range(before[9], before[9] + 7))


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """One lqer_kv_pool_copy with fixed id tensors captured (one launch: a linear capture) and replayed twice, the second time after the
    source changed: each time the destination's bytes are those of the eager call into a twin of the destination."""
    from lqer_amd.kvcache import pool_copy

    dtype, d, bits = FORMS[4]
    src, seqs = source(dtype, d, bits)
    dst, twin = (make(dtype, d, bits, pages=16, slots=9) for _ in range(2))
    pages = list(dict.fromkeys(p for s in seqs[3:] for p in held(src, s)))
    slots = [src.pt.slot(s) for s in seqs[3:]]
    n, m = len(pages), len(slots)
    ids = torch.tensor(pages + [15 - i for i in range(n)] + slots + [8 - j for j in range(m)], dtype=torch.int32).to(DEV)
    args = lambda to: (src.buf, src.pt.num_pages, src.pt.max_seqs, to.buf, 16, 9, dtype, HK, d, ids, n, m, *src._code_fmts())
    pool_copy(*args(twin))
    pool_copy(*args(dst))  # (the first launch of a kernel loads its code: not under capture)
    torch.cuda.synchronize()
    assert torch.equal(dst.buf, twin.buf) and not bool((twin.buf == 0xFF).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pool_copy(*args(dst))
    for round_ in range(2):
        if round_:
            first = twin.buf.clone()
            src.append(seqs[3:], *kv(9, d, dtype, 800, batch=4))  # the open blocks and the staging rows change, under the same ids
            pool_copy(*args(twin))
            assert not torch.equal(twin.buf, first)
        dst.buf.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst.buf, twin.buf), f"replay {round_}"

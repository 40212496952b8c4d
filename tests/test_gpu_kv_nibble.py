"""Nibble code storage of the paged KV pool on the GPU (LQER_Q_MXINT_C4: include/lqer_hip.h "paged KV pool", nibble codes; the N4 / K4 /
V4 instantiations of csrc/kv_cache.hip and csrc/attn_decode.hip; lqer_amd.kvcache.PagedKVCache(code_bits=...)).

The storage changes no rounding, so nothing here has a tolerance: the stored nibbles are the oracle's sign and magnitude by the
header's layout (case 1 - every other case would pass with a self-consistent wrong layout), and everything else is torch.equal against
a pool of BYTE codes of the same formats that was fed the same K and V.  Both pools start as 0xFF: a stale neighbour nibble, a page
read beyond a length or below a window shows.  K^T and V are the formats' ladders (tests/_formats.py), asserted on the CPU to reach
every class of exponent the dtype holds before the first GPU call."""
import ctypes as C

import pytest
import torch

import _attention as A
import _formats as F
import _guard
from oracle import lqer_oracle as O

pytestmark = pytest.mark.gpu

DEV = A.DEV
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
FMTS = [("e8", 4), ("e4", 4), ("e3b6", 4), ("e4", 3), ("e4", 2)]  # (exponent field, width)
GEOMS = [(16, 4, 4), (48, 4, 2), (128, 4, 4), (16, 4, 2), (48, 4, 4), (128, 4, 2)]  # (d, heads, kv_heads)
# every format with every dtype, the six geometries in turn: each d five times, each head ratio with every format
COMBOS = [pytest.param(f, dt, GEOMS[(3 * i + j) % 6], id=f"{f[0]}w{f[1]}-{dt}-d{GEOMS[(3 * i + j) % 6][0]}h{GEOMS[(3 * i + j) % 6][2]}")
          for i, f in enumerate(FMTS) for j, dt in enumerate(DTYPES)]
# one case per format for the attention cases, which loop over the call shapes: all dtypes, all d, both head ratios
ATT = [pytest.param(f, dt, g, id=f"{f[0]}w{f[1]}-{dt}-d{g[0]}h{g[2]}") for f, dt, g in
       ((FMTS[0], "f16", GEOMS[5]), (FMTS[1], "bf16", GEOMS[1]), (FMTS[2], "f32", GEOMS[0]), (FMTS[3], "f16", GEOMS[4]), (FMTS[4], "bf16", GEOMS[2]),
        (FMTS[1], "f32", GEOMS[5]))]

u8 = lambda t: t.contiguous().view(torch.uint8)
pages_of = lambda n: (n + 15) // 16


def same(a, b, what=""):
    assert torch.equal(u8(a), u8(b)), f"{what}: {(u8(a) != u8(b)).sum().item()} of {u8(a).numel()} bytes differ from the byte pool's"


def kv_cfgs(k, v):
    x = F.cfg("e8", 8, [1, 16], True)
    return (dict(name="flexible", default=x, x_quantizer=x, w_quantizer=F.cfg(*k, [1, 16], True)),
            dict(name="flexible", default=x, x_quantizer=x, w_quantizer=F.cfg(*v, [1, 16], True)))


def kv_ladder(fk, fv, dtype, hk, t, d, seed):
    """K whose transposed rows [d, t] and V whose rows [t, d] are format ladders, [1, hk, t, d] each."""
    kt = F.ladder(fk, dtype, hk * d, t, 16, seed=seed)
    v = F.ladder(fv, dtype, hk * t, d, 16, seed=seed + 1)
    return kt.reshape(1, hk, d, t).transpose(2, 3).contiguous(), v.reshape(1, hk, t, d).contiguous()


_RAWS = {}


def raws_for(k, v, dtype, hk, d, lens, seed=0):
    """One (K, V) per length on the GPU, made once per key and never changed; the long ones are asserted to cover the formats' classes."""
    key = (k, v, dtype, hk, d, tuple(lens), seed)
    if key not in _RAWS:
        cfg0, cfg1 = kv_cfgs(k, v)
        out = []
        for i, n in enumerate(lens):
            kk, vv = kv_ladder(k[0], v[0], dtype, hk, n, d, seed=7000 + 100 * seed + i)
            if n >= 37:
                F.assert_covered(kk.reshape(hk, n, d).transpose(1, 2).contiguous(), k[0], cfg0["w_quantizer"], dtype)
                F.assert_covered(vv.reshape(hk * n, d), v[0], cfg1["w_quantizer"], dtype)
            out.append((kk, vv))
        _RAWS[key] = [(a.to(DEV), b.to(DEV)) for a, b in out], out
    return _RAWS[key]


def pool(k, v, dtype, hk, d, pages, slots, bits, room, **kw):
    """A pool of 0xFF bytes: pages and slots are reused dirty, and here they start so."""
    from lqer_amd import PagedKVCache

    cache = PagedKVCache(pages, slots, hk, d, *kv_cfgs(k, v), dtype, DEV, max_pages_per_seq=room, code_bits=bits, **kw)
    cache.buf.fill_(0xFF)
    return cache


def fill(cache, raws, steps_of):
    """One sequence per (K, V), appended in the pieces steps_of(length) names: the sequences."""
    seqs = []
    for kk, vv in raws:
        n, at = kk.shape[2], 0
        seqs.append(cache.alloc())
        for s in steps_of(n):
            cache.append([seqs[-1]], kk[:, :, at:at + s], vv[:, :, at:at + s])
            at += s
        assert at == n == cache.length(seqs[-1])
    return seqs


def two_pools(k, v, dtype, hk, d, lens, steps_of=lambda n: [n], bits=4, spare=0, seed=0, **kw):
    """(the pool with `bits`, the byte pool) of the same formats, fed the same K and V in the same pieces; their sequences; the raws."""
    raws, _ = raws_for(k, v, dtype, hk, d, lens, seed)
    out = []
    for b in (bits, None):
        cache = pool(k, v, dtype, hk, d, sum(map(pages_of, lens)) + spare, len(lens) + spare, b, max(map(pages_of, lens)) + 1, **kw)
        out.append((cache, fill(cache, raws, steps_of)))
    (nib, ns), (byt, bs) = out
    assert nib.nibble and not byt.nibble and nib.nbytes < byt.nbytes
    assert ns == bs and nib.pt.table == byt.pt.table and nib.pt.released == byt.pt.released  # the same books
    return nib, byt, ns, raws


# ---- the header's layout, restated -------------------------------------------------------------------------------------------------------
def sections(cache):
    """Byte offsets {name: (offset, bytes of an item)} of the pool's four code and exponent sections, each rounded up to 256 bytes; a
    code row is D bytes, or D / 2 where the operand's codes are nibbles."""
    up = lambda x: (x + 255) // 256 * 256
    d, items = cache.head_dim, cache.pt.num_pages * cache.kv_heads
    out, at = {}, 0
    for name, per in (("k_codes", 16 * d * cache.code_bits[0] // 8), ("k_exps", d), ("v_codes", 16 * d * cache.code_bits[1] // 8), ("v_exps", d)):
        out[name] = (at, per)
        at += up(items * per)
    esz = torch.empty((), dtype=cache.dtype).element_size()
    assert at + up(cache.pt.max_seqs * cache.kv_heads * 16 * d * esz) == cache.nbytes
    return out


def items_of(cache, host, seq, name):
    """[kv_heads, blocks, bytes of an item] of one section for the blocks of 16 keys of a sequence: item page * kv_heads + g."""
    at, per = sections(cache)[name]
    row = cache.pt.table[cache.pt.slot(seq)][:pages_of(cache.length(seq))]
    sec = host[at:at + cache.pt.num_pages * cache.kv_heads * per].view(cache.pt.num_pages, cache.kv_heads, per)
    return sec[torch.tensor(row, dtype=torch.int64)].permute(1, 0, 2).contiguous()


def stored_codes(cache, host, seq, which):
    """(sign, magnitude) [kv_heads, T, D] int32 of K ("k") or V ("v"): codes [16][D] bytes - bit 7 the sign -, or [16][D / 2] bytes of
    nibbles - elements 2 j and 2 j + 1 the low and the high nibble of byte j, a nibble sign << 3 | magnitude."""
    d, t = cache.head_dim, cache.length(seq)
    x = items_of(cache, host, seq, which + "_codes").to(torch.int32)
    hk, nb, _ = x.shape
    if cache.code_bits[0 if which == "k" else 1] == 4:
        x = x.view(hk, nb, 16, d // 2)
        n = torch.stack([x & 15, x >> 4], dim=-1).reshape(hk, nb * 16, d)[:, :t]
        return n >> 3, n & 7
    x = x.view(hk, nb * 16, d)[:, :t]
    return x >> 7, x & 127


def stored_exps(cache, host, seq):
    """K exponent bytes [kv_heads, blocks, D] and V exponent bytes [kv_heads, T, D / 16] (stored at [block][D / 16][16])."""
    d, t = cache.head_dim, cache.length(seq)
    ke = items_of(cache, host, seq, "k_exps").to(torch.int32)
    ve = items_of(cache, host, seq, "v_exps").to(torch.int32)
    hk, nb, _ = ve.shape
    return ke, ve.view(hk, nb, d // 16, 16).permute(0, 1, 3, 2).reshape(hk, nb * 16, d // 16)[:, :t]


def check_against_oracle(nib, byt, seq, raw_cpu, k, v, t):
    """The first t keys of raw_cpu are what `seq` holds: nibbles and exponent bytes against the oracle, the sign against the byte pool."""
    assert nib.length(seq) == byt.length(seq) == t
    hn, hb = nib.buf.cpu(), byt.buf.cpu()
    cfg0, cfg1 = kv_cfgs(k, v)
    hk, d = nib.kv_heads, nib.head_dim
    kk, vv = (x[0, :, :t].float() for x in raw_cpu)
    kt = kk.transpose(1, 2).contiguous()  # [hk, d, t]: the K quantizer's blocks run along the keys
    negzero = 0
    for which, src, fid, c in (("k", kt.reshape(hk * d, t), k[0], cfg0["w_quantizer"]), ("v", vv.reshape(hk * t, d), v[0], cfg1["w_quantizer"])):
        _, codes, e = F.oracle_q(src, c, decompose=True)
        codes = codes.reshape(hk, d, t).transpose(1, 2) if which == "k" else codes.reshape(hk, t, d)
        x = kk if which == "k" else vv
        sign, mag = stored_codes(nib, hn, seq, which)
        bsign, bmag = stored_codes(byt, hb, seq, which)
        assert torch.equal(mag, codes.abs()), f"{which} at {t} keys: {(mag != codes.abs()).sum().item()} magnitudes differ from the oracle's"
        assert torch.equal(sign[codes != 0], (codes < 0).int()[codes != 0]), f"{which} at {t} keys: signs differ from the oracle's"
        assert torch.equal(bmag, mag) and torch.equal(sign, bsign), f"{which} at {t} keys: sign or magnitude differs from the byte pool's"
        negzero += int(((codes == 0) & (x < 0) & (x.abs() > 1e-8)).sum())  # negative values that round to zero: the sign is bit 7's (above)
        emin, emax = F.e_range(fid)
        blk, _ = O._blocks(src, c["block_size"], True)
        e = torch.where(blk.abs().amax(dim=-1) != 0, e, torch.full_like(e, min(max(0, emin), emax))) - emin
        ke, ve = stored_exps(nib, hn, seq)
        if which == "k":
            assert torch.equal(ke, e.reshape(hk, d, pages_of(t)).permute(0, 2, 1).int()), f"K exponent bytes at {t} keys"
        else:
            assert torch.equal(ve, e.reshape(hk, t, d // 16).int()), f"V exponent bytes at {t} keys"
    return negzero


# ---- 1. stored bytes against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f, dt, geom", COMBOS)
def test_stored_nibbles_are_the_oracles_sign_and_magnitude(f, dt, geom):
    """Three sequences to 37 keys - one token at a time, 20 + 17, one chunk of 37 -, read back at lengths 1, 15, 16, 17 (20) and 37."""
    dtype, (d, _, hk) = DTYPES[dt], geom
    (raw,), (raw_cpu,) = raws_for(f, f, dtype, hk, d, [37])
    nib, byt = (pool(f, f, dtype, hk, d, 9, 3, b, 3) for b in (4, None))
    negzero = 0
    for steps, stops in (([1] * 37, (1, 15, 16, 17, 37)), ([20, 17], (20, 37)), ([37], (37,))):
        sn, sb = nib.alloc(), byt.alloc()
        at = 0
        for s in steps:
            for cache, seq in ((nib, sn), (byt, sb)):
                cache.append([seq], raw[0][:, :, at:at + s], raw[1][:, :, at:at + s])
            at += s
            if at in stops:
                negzero += check_against_oracle(nib, byt, sn, raw_cpu, f, f, at)
    assert negzero > 0  # (the ladder holds negative values that round to zero)


# ---- 2. gather ------------------------------------------------------------------------------------------------------------------------------
def dense_live(dense, t):
    """The live part of each section of a dense cache of batch 1: codes and exponents up to t keys, staging rows up to t % 16."""
    from lqer_amd import kvcache

    hk, d, cap = dense.kv_heads, dense.head_dim, dense.capacity
    esz = torch.empty((), dtype=dense.dtype).element_size()
    secs, _ = kvcache._sections(dense.dtype, 1, hk, cap, d)
    at = {name: off for name, off, _ in secs}
    b = dense.buf
    return [b[at["k_codes"]:at["k_codes"] + hk * cap * d].view(hk, cap, d)[:, :t],
            b[at["k_exps"]:at["k_exps"] + hk * (cap // 16) * d].view(hk, cap // 16, d)[:, :pages_of(t)],
            b[at["v_codes"]:at["v_codes"] + hk * cap * d].view(hk, cap, d)[:, :t],
            b[at["v_exps"]:at["v_exps"] + hk * (cap // 16) * d].view(hk, cap // 16, d // 16, 16).permute(0, 1, 3, 2).reshape(hk, cap, d // 16)[:, :t],
            b[at["k_stage"]:at["k_stage"] + hk * 16 * d * esz].view(hk, 16, d * esz)[:, :t % 16]]


@pytest.mark.parametrize("bits", [4, (4, 8), (8, 4)], ids=["K4V4", "K4V8", "K8V4"])
@pytest.mark.parametrize("f, dt, geom", ATT)
def test_gather_writes_the_byte_pools_dense_cache(f, dt, geom, bits):
    dtype, (d, _, hk) = DTYPES[dt], geom
    lens = (1, 16, 17, 300)
    nib, byt, seqs, _ = two_pools(f, f, dtype, hk, d, lens, lambda n: [n - n // 3, n // 3] if n > 2 else [n], bits=bits)
    for seq, t in zip(seqs, lens):
        a, b = nib.to_dense(seq), byt.to_dense(seq)
        assert a.buf.numel() == b.buf.numel() and a.length == b.length == t
        for x, y, name in zip(dense_live(a, t), dense_live(b, t), ("K codes", "K exponents", "V codes", "V exponents", "staging rows")):
            same(x, y, f"{name} of the dense cache at {t} keys")
        for x, y in zip(nib.dequantized(seq), byt.dequantized(seq)):
            same(x, y, f"dequantized at {t} keys")


# ---- 3. chunked appends against one append -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f, dt, geom", COMBOS)
def test_chunked_appends_leave_the_bytes_of_one_append(f, dt, geom):
    """1 + 15 + 1 + 20 keys against 37 at once, on pools of 0xFF: every rewrite of an open block stores whole bytes over all 16 rows, so
    no stale nibble is left - the K items (all rows: the padding is codes of 0) and the live V rows and exponents are equal."""
    dtype, (d, _, hk) = DTYPES[dt], geom
    (raw,), _ = raws_for(f, f, dtype, hk, d, [37])
    hosts = []
    for steps in ([1, 15, 1, 20], [37]):
        cache = pool(f, f, dtype, hk, d, 3, 1, 4, 3)
        seq, = fill(cache, [raw], lambda n: steps)
        hosts.append((cache, cache.buf.cpu(), seq))
    (ca, ha, sa), (cb, hb, sb) = hosts
    for name in ("k_codes", "k_exps"):
        assert torch.equal(items_of(ca, ha, sa, name), items_of(cb, hb, sb, name)), name
    for which in ("k", "v"):
        for x, y in zip(stored_codes(ca, ha, sa, which), stored_codes(cb, hb, sb, which)):
            assert torch.equal(x, y), which
    va, vb = items_of(ca, ha, sa, "v_codes").view(hk, 48, d // 2)[:, :37], items_of(cb, hb, sb, "v_codes").view(hk, 48, d // 2)[:, :37]
    assert torch.equal(va, vb)
    for x, y in zip(stored_exps(ca, ha, sa), stored_exps(cb, hb, sb)):
        assert torch.equal(x, y)
    # the open block's rows beyond the length: zero codes (0x00 bytes), not the 0xFF the page held
    kc = items_of(ca, ha, sa, "k_codes").view(hk, 48, d // 2)
    assert bool((kc[:, 37:] == 0).all())


# ---- 4. decode ------------------------------------------------------------------------------------------------------------------------------
LENS = (1, 15, 16, 17, 37, 300, 2049)
ORDER = (4, 0, 6, 2, 5, 1, 3)  # the call's order of the sequences: not the slots'


def steps2(n):
    return [n - 5, 5] if n > 5 else [n]  # (on a windowed cache the second append releases pages)


def att(q, cache, seqs, causal, **kw):
    from lqer_amd import attention_flexible_paged

    return attention_flexible_paged(q, cache, seqs, q.shape[3] ** -0.5, causal=causal, return_stats=True, **kw)


def queries(shape, dtype, seed):
    return A._randn(shape, dtype, seed, 2.0 ** -10).to(DEV)  # (small: the scores of the ladders' large keys stay inside fp16)


@pytest.mark.parametrize("f, dt, geom", ATT)
def test_decode_equals_the_byte_pool(f, dt, geom):
    """S = 1, 3, 8 with and without the causal rule (causal: the sequences that hold at least S keys) over the ragged batch in shuffled
    order, then per-sequence counts 1 .. 8 through the ragged decode call."""
    from lqer_amd import attention_flexible_paged_decode_ragged

    dtype, (d, h, hk) = DTYPES[dt], geom
    nib, byt, seqs, _ = two_pools(f, f, dtype, hk, d, LENS, steps2)
    for s in (1, 3, 8):
        for causal in (False, True):
            call = [seqs[i] for i in ORDER if not causal or LENS[i] >= s]
            q = queries((len(call), h, s, d), dtype, 10 + s)
            (a, sa), (b, sb) = att(q, nib, call, causal), att(q, byt, call, causal)
            same(a, b, f"out S={s} causal={causal}"), same(sa, sb, f"row_stats S={s} causal={causal}")
    for counts in ((1, 2, 3, 4, 5, 6, 7), (1, 8, 7, 6, 5, 4, 3), (0, 1, 8, 0, 2, 1, 1)):
        pick = sorted(range(7), key=lambda i: (LENS[i], i))  # counts in the order of the lengths: every count <= its length
        call, cs = [seqs[pick[j]] for j in ORDER], [counts[j] for j in ORDER]
        q = queries((sum(cs), h, d), dtype, 20 + counts[1])
        (a, sa), (b, sb) = (attention_flexible_paged_decode_ragged(q, c, call, cs, d ** -0.5, causal=True, return_stats=True) for c in (nib, byt))
        same(a, b, f"out counts={cs}"), same(sa, sb, f"row_stats counts={cs}")


@pytest.mark.parametrize("window", [20, 200])
@pytest.mark.parametrize("f, dt, geom", ATT[:3] + ATT[4:5])
def test_windowed_decode_equals_the_byte_pool(f, dt, geom, window):
    """Caches with a window: the second append of every sequence releases the pages nothing can see, the window cuts inside a page."""
    from lqer_amd import attention_flexible_paged_decode_ragged

    dtype, (d, h, hk) = DTYPES[dt], geom
    nib, byt, seqs, _ = two_pools(f, f, dtype, hk, d, LENS, steps2, window=window)
    assert nib.pt.released[nib.pt.slot(seqs[6])] == (2049 - window - 7) // 16 > 0
    assert nib.pt.released[nib.pt.slot(seqs[5])] == (300 - window - 7) // 16 > 0
    for s in (1, 3, 8):
        call = [seqs[i] for i in ORDER if LENS[i] >= s]
        q = queries((len(call), h, s, d), dtype, 30 + s)
        (a, sa), (b, sb) = att(q, nib, call, True), att(q, byt, call, True)
        same(a, b, f"out S={s} window={window}"), same(sa, sb, f"row_stats S={s} window={window}")
    cs = [(1, 2, 3, 4, 5, 6, 7)[j] for j in ORDER]
    call = [seqs[j] for j in ORDER]  # (LENS is ascending: count j + 1 <= LENS[j])
    q = queries((sum(cs), h, d), dtype, 39)
    (a, sa), (b, sb) = (attention_flexible_paged_decode_ragged(q, c, call, cs, d ** -0.5, causal=True, return_stats=True) for c in (nib, byt))
    same(a, b, f"out counts={cs} window={window}"), same(sa, sb, f"row_stats counts={cs} window={window}")


# ---- 5. the prefill route -------------------------------------------------------------------------------------------------------------------
PLENS = (37, 300, 129, 200)


@pytest.mark.parametrize("f, dt, geom", ATT)
def test_prefill_equals_the_byte_pool(f, dt, geom):
    from lqer_amd import attention_flexible_paged_ragged

    dtype, (d, h, hk) = DTYPES[dt], geom
    nib, byt, seqs, _ = two_pools(f, f, dtype, hk, d, PLENS, steps2)
    for s, causal in ((9, False), (9, True), (70, False)):
        q = queries((3, h, s, d), dtype, 40 + s)
        (a, sa), (b, sb) = (att(q, c, seqs[:3], causal, kernel="prefill") for c in (nib, byt))
        same(a, b, f"out S={s} causal={causal}"), same(sa, sb, f"row_stats S={s} causal={causal}")
    counts = (1, 1, 33, 129)
    q = queries((sum(counts), h, d), dtype, 49)
    for kernel in ("auto", "prefill"):
        (a, sa), (b, sb) = (attention_flexible_paged_ragged(q, c, seqs, counts, d ** -0.5, causal=True, return_stats=True, kernel=kernel) for c in (nib, byt))
        same(a, b, f"out counts={counts} {kernel}"), same(sa, sb, f"row_stats counts={counts} {kernel}")


@pytest.mark.parametrize("f, dt, geom", ATT[1:4])
def test_windowed_prefill_equals_the_byte_pool(f, dt, geom):
    """Window 64 on a cache made for 72 query rows: 70 rows per sequence through lqer_attention_q_paged_window, pages below released."""
    dtype, (d, h, hk) = DTYPES[dt], geom
    nib, byt, seqs, _ = two_pools(f, f, dtype, hk, d, (300, 129, 200), steps2, window=64, max_query_rows=72)
    assert nib.pt.released[nib.pt.slot(seqs[0])] > 0
    q = queries((3, h, 70, d), dtype, 50)
    names = []
    from lqer_amd import kvcache

    real = kvcache._paged_args
    try:
        kvcache._paged_args = lambda *a, **kw: (lambda r: (names.append(r[0]), r)[1])(real(*a, **kw))
        (a, sa), (b, sb) = (att(q, c, seqs, True, kernel="prefill") for c in (nib, byt))
    finally:
        kvcache._paged_args = real
    assert names == ["lqer_attention_q_paged_window"] * 2
    same(a, b, "out"), same(sa, sb, "row_stats")


# ---- 6. mixed storage -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, k, v", [((4, 8), ("e4", 4), ("e5b20", 8)), ((8, 4), ("e5b20", 8), ("e3b6", 3))], ids=["K4V8", "K8V4"])
def test_mixed_storage(bits, k, v):
    """One operand in nibbles beside a wide one in bytes: the stored codes of both against the oracle, one decode and one prefill call."""
    dtype, d, h, hk = torch.bfloat16, 48, 4, 2
    lens = (37, 300)
    nib, byt, seqs, _ = two_pools(k, v, dtype, hk, d, lens, steps2, bits=bits)
    assert nib.code_bits == bits
    _, raws_cpu = raws_for(k, v, dtype, hk, d, lens)
    for seq, raw_cpu, t in zip(seqs, raws_cpu, lens):
        check_against_oracle(nib, byt, seq, raw_cpu, k, v, t)
    q = queries((2, h, 3, d), dtype, 60)
    (a, sa), (b, sb) = att(q, nib, seqs, True), att(q, byt, seqs, True)
    same(a, b, "decode out"), same(sa, sb, "decode row_stats")
    q = queries((2, h, 20, d), dtype, 61)
    (a, sa), (b, sb) = (att(q, c, seqs, True, kernel="prefill") for c in (nib, byt))
    same(a, b, "prefill out"), same(sa, sb, "prefill row_stats")


# ---- 7. fork --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lp", [17, 32], ids=["open-block", "no-open-block"])
@pytest.mark.parametrize("f, dt, geom", ATT[:5])
def test_fork_children_attend_with_the_byte_pools_bits(f, dt, geom, lp):
    """fork_many at 17 keys (an open block: the item, at the size the formats give it, and the staging rows are copied) and at 32 (none);
    the children are appended different keys.  shared_prefix=True runs the ungrouped call on the nibble pool: the same bits."""
    from lqer_amd import kvcache

    dtype, (d, h, hk) = DTYPES[dt], geom
    raws, _ = raws_for(f, f, dtype, hk, d, [lp, 3, 21, 6], seed=lp)
    outs = []
    for bits in (4, None):
        cache = pool(f, f, dtype, hk, d, 12, 4, bits, 4)
        parent, = fill(cache, raws[:1], lambda n: [n])
        kids = cache.fork_many([parent, parent])
        for seq, (kk, vv) in zip([parent] + kids, raws[1:]):
            cache.append([seq], kk, vv)
        seqs = [kids[1], parent, kids[0]]
        assert [cache.length(x) for x in seqs] == [lp + 6, lp + 3, lp + 21]
        q = queries((3, h, 3, d), dtype, 70)
        names, real = [], kvcache._paged_args
        try:
            kvcache._paged_args = lambda *a, **kw: (lambda r: (names.append(r[0]), r)[1])(real(*a, **kw))
            plain, grouped = att(q, cache, seqs, True), att(q, cache, seqs, True, shared_prefix=True)
        finally:
            kvcache._paged_args = real
        assert names == [kvcache.PAGED_DECODE, kvcache.PAGED_DECODE if bits else kvcache.SHARED_DECODE]
        same(grouped[0], plain[0], "shared_prefix out"), same(grouped[1], plain[1], "shared_prefix row_stats")
        outs.append(plain + tuple(x for seq in seqs for x in cache.dequantized(seq)))
    for a, b in zip(*outs):
        same(a, b, f"fork at {lp}")


# ---- 8. guard zones -------------------------------------------------------------------------------------------------------------------------
def _guarded_run(fill_byte, bits):
    """Appends (uniform and ragged), a fork, a gather, one decode and one prefill call on a pool of EXACTLY lqer_kv_pool_bytes_fmt bytes
    between guards: every output, for the comparison across fills."""
    from lqer_amd import _lib, attention_flexible_paged, ops

    L = _lib.lib()
    f, dtype, d, h, hk, stride = ("e4", 4), torch.float16, 48, 4, 2, 4
    cache = pool(f, f, dtype, hk, d, 11, 5, bits, stride)
    assert cache.nbytes == L.lqer_kv_pool_bytes_fmt(_lib.F16, 11, 5, hk, d, C.byref(cache.fmts[1]), C.byref(cache.fmts[3]))
    if bits is not None:
        assert cache.nbytes < L.lqer_kv_pool_bytes(_lib.F16, 11, 5, hk, d)  # (a kernel left on byte strides writes past it)
    g_pool = _guard.guarded(cache.nbytes, align=16, fill=fill_byte, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(5, stride)
    raws, _ = raws_for(f, f, dtype, hk, d, [41, 35, 18, 5, 9])
    lens = (41, 35, 18)
    g_in = [_guard.guarded(x.numel() * 2, align=16, name=nm).load(x) for kv in raws for x, nm in zip(kv, ("k_new", "v_new"))]
    kv = [(g_in[2 * i].view(dtype).view(raws[i][0].shape), g_in[2 * i + 1].view(dtype).view(raws[i][1].shape)) for i in range(5)]
    seqs = [cache.alloc() for _ in lens]
    for s, (kk, vv) in zip(seqs, kv):  # uniform appends, in two pieces
        cache.append([s], kk[:, :, :7], vv[:, :, :7])
        cache.append([s], kk[:, :, 7:], vv[:, :, 7:])
    # a ragged append: 5, 0 and 9 more keys, packed [total][kv_heads][d]
    packed = [_guard.guarded(14 * hk * d * 2, align=16, name=nm).load(torch.cat([kv[3][j][0].transpose(0, 1), kv[4][j][0].transpose(0, 1)]).contiguous())
              for j, nm in ((0, "k_new (ragged)"), (1, "v_new (ragged)"))]
    cache.append_ragged(seqs, *(g.view(dtype).view(14, hk, d) for g in packed), [5, 0, 9])
    kid, = cache.fork(seqs[2])  # 27 keys: an open block
    cache.append([kid], kv[3][0], kv[3][1])
    torch.cuda.synchronize()
    g_pool.check(), g_tbl.check()
    call, T = seqs + [kid], [46, 35, 27, 32]
    assert [cache.length(s) for s in call] == T
    # gather: the raw call into a dense cache of exactly lqer_kv_cache_bytes between guards
    g_dense = _guard.guarded(L.lqer_kv_cache_bytes(_lib.F16, 1, hk, 48, d), align=16, fill=fill_byte, name="dense cache")
    name, fmts = cache._with_code_fmts("lqer_kv_pool_gather")
    pool_before = g_pool.payload.clone()
    _lib.check(getattr(L, name)(cache.buf.data_ptr(), cache.nbytes, _lib.F16, 11, 5, hk, d, cache.table.data_ptr(), stride, cache.pt.slot(seqs[0]), 46,
                                g_dense.ptr, g_dense.nbytes, 48, *fmts, ops._stream(torch.device(DEV))), name)
    outs = []
    for s, kernel in ((3, "decode"), (20, "prefill")):
        g_q = _guard.guarded(4 * h * s * d * 2, align=16, name="q").load(queries((4, h, s, d), dtype, 80 + s))
        size = L.lqer_attention_q_decode_paged_workspace_bytes(4, h, hk, s, cache.pt.max_len, d) if kernel == "decode" else \
            L.lqer_attention_q_paged_workspace_bytes(4, h, hk, s, min(128, cache.pt.max_len), d)
        g_ws = _guard.guarded(size, align=16, fill=0xFF, name="workspace")
        out, st = attention_flexible_paged(g_q.view(dtype).view(4, h, s, d), cache, call, d ** -0.5, causal=True, return_stats=True, kernel=kernel,
                                           ws=g_ws.payload)
        torch.cuda.synchronize()
        g_ws.check(), g_q.unchanged()
        outs += [out, st]
    torch.cuda.synchronize()
    g_pool.check(), g_tbl.check(), g_dense.check()
    for g in g_in + packed:
        g.unchanged()
    assert torch.equal(g_pool.payload, pool_before)  # gather and attention only read the pool
    from lqer_amd import QuantizedKVCache

    dense = QuantizedKVCache(1, hk, d, cache.cfg0, cache.cfg1, dtype, DEV, capacity=48)
    dense.buf, dense.length = g_dense.payload, 46
    return outs + dense_live(dense, 46) + [x for s in call for x in cache.dequantized(s)]


@pytest.mark.parametrize("bits", [4, (4, 8), (8, 4)], ids=["K4V4", "K4V8", "K8V4"])
def test_guard_zones_and_fills(bits):
    """Over a pseudo-random fill and over 0xFF: guards and inputs stay bit-unchanged, every output is the same over both fills - and
    the byte pool's."""
    runs = [_guarded_run(fill_byte, bits) for fill_byte in (3, 0xFF)] + [_guarded_run(0xFF, None)]
    for i, (a, b, c) in enumerate(zip(*runs)):
        same(a, b, f"output {i} over the two fills"), same(a, c, f"output {i}")


# ---- 9. capture -----------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """One decode call on the nibble pool captured on one stream (a linear capture: three launches, no parallel branches), replayed with
    changed q and lengths: the eager call's bits."""
    from lqer_amd import _lib, kvcache, ops
    from test_kv_paged_call_cpu import _names

    f, dtype, d, h, hk, s = ("e4", 4), torch.float16, 48, 4, 2, 3
    lens = (37, 300, 17)
    nib, byt, seqs, _ = two_pools(f, f, dtype, hk, d, lens)
    slots = nib.pt.slots(seqs)
    L = _lib.lib()
    q = queries((3, h, s, d), dtype, 90)
    out, st = torch.empty_like(q), torch.empty(3, h, s, 2, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.lqer_attention_q_decode_paged_workspace_bytes(3, h, hk, s, nib.pt.max_len, d), dtype=torch.uint8, device=DEV)
    # the metadata goes up before the capture; the recorded call takes the capture's stream
    name, args = kvcache._paged_args(kvcache.PAGED_DECODE, q, out, st, nib, slots, list(lens), d ** -0.5, True, None, ws.data_ptr(), ws.numel(), None, S=s)
    assert name == kvcache.PAGED_DECODE
    at = _names(name).index("stream")
    call = lambda: _lib.check(getattr(L, name)(*args[:at], ops._stream(q.device), *args[at + 1:]), name)
    call()
    torch.cuda.synchronize()
    want, want_st = att(q, byt, seqs, True)
    same(out, want, "eager out"), same(st, want_st, "eager row_stats")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seed, now in ((90, lens), (91, (20, 257, 16))):  # shorter lengths: the keys are there, the chunk length of the second changes
        q.copy_(queries((3, h, s, d), dtype, seed))
        nib._lens[:3].copy_(torch.tensor(now, dtype=torch.int32))
        out.fill_(0), st.fill_(0), ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        got, got_st = out.clone(), st.clone()
        kvcache._paged_args(kvcache.PAGED_DECODE, q, out, st, nib, slots, list(now), d ** -0.5, True, None, ws.data_ptr(), ws.numel(), None, S=s)
        out.fill_(0), st.fill_(0)
        call()  # the eager call at these lengths
        torch.cuda.synchronize()
        same(got, out, f"replay {seed} out"), same(got_st, st, f"replay {seed} row_stats")
        if now == lens:
            same(got, want, "replay out"), same(got_st, want_st, "replay row_stats")
        else:
            assert not torch.equal(u8(got), u8(want))

"""A draft tree per sequence on the paged KV pool, on the GPU (lqer_attention_q_decode_paged_tree: k_attn_dec_scores_tree /
k_attn_dec_pv_tree of csrc/attn_decode.hip; lqer_attention_q_paged_tree: k_attn_q_tree of csrc/attn_q.hip; attention_flexible_paged_tree).

The contract is an equality of bits per sequence: the rows of sequence b in out and row_stats are those of ONE batch-1 call on the raw
K and V of that sequence - the context plus all its draft nodes - with the tree as an additive mask tensor, 0 where a row sees a key
and torch.finfo(dtype).min elsewhere: attention_flexible(q_b, K_b, V_b, ..., attention_mask=M, kernel="decode") for trees of up to 8
nodes, kernel="prefill" beyond - never the paged code itself.  Every comparison is torch.equal on the bytes; there is no tolerance in
this file.

The decode route - (keys, nodes): (8, 8) base 0, no context; (17, 8) draft keys 9 .. 16 over the page and chunk edge at 16; (33, 1);
(257, 6) chunks of 32, draft keys 251 .. 256 over key 256; (2049, 8) the last 128-key chunk holds draft node 7 alone - no visible key
there for a row without bit 7; (40, 0) a sequence that is left out.  Geometries d 48 heads 4 / 2, d 128 heads 16 / 2 (rep 8: 8, 48
and 64 rows per kv head, on both sides of the 32-row group), d 64 heads 8 / 8.  Trees: chain, star, binary, two roots; the single
node is sequence 2 of every set.
The prefill route - (64, 64) base 0, row 63's bit 63; (70, 9) the smallest count the decode route does not take, draft keys 61 .. 69
over the 64-key tile; (100, 33) one row in the second wave, the region over the 32-key subtile at 96; (321, 64) key 320 alone in its
tile.  Geometries d 16 heads 2 / 1, d 48 heads 4 / 2, d 128 heads 16 / 2.  Trees: chain, star, heap (parent = (i - 1) // 2) and a
26-node tree three levels deep (two roots, fan-out 3), the last with 26 nodes on every length.
tests/test_kv_tree_cpu.py holds the arithmetic that says the sets reach these edges."""
import ctypes as C
import functools

import pytest
import torch

import _guard
import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
from test_gpu_kv_paged import pages_of, u8
from test_gpu_kv_ragged import _padded, starts_of

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES = F.CFG, F.DEV, F.DTYPES
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
F16 = torch.float16
DECODE, PREFILL = "lqer_attention_q_decode_paged_tree", "lqer_attention_q_paged_tree"
# route -> the sequences of its pool as (keys, nodes), its geometries (d, heads, kv heads), its comparator's kernel
SETS = {"dec": ((8, 8), (17, 8), (33, 1), (257, 6), (2049, 8), (40, 0)),
        "pre": ((64, 64), (70, 9), (100, 33), (321, 64))}
GEOM = {"dec": {"d48": (48, 4, 2), "d128": (128, 16, 2), "d64": (64, 8, 8)},
        "pre": {"d16": (16, 2, 1), "d48": (48, 4, 2), "d128": (128, 16, 2)}}
KERNEL = {"dec": "decode", "pre": "prefill"}
# a tree of n nodes by its name: the parents, parents before children
TREES = {"chain": lambda n: tuple(range(-1, n - 1)),
         "star": lambda n: (-1,) * n,
         "binary": lambda n: tuple((i - 1) // 2 for i in range(n)),           # [-1, 0, 0, 1, 1, 2, 2, 3]; 64 nodes: the heap
         "tworoots": lambda n: (-1, -1)[:n] + tuple(range(max(n - 2, 0))),     # [-1, -1, 0, 1, 2, 3]: two chains side by side
         "deep26": lambda n: tuple(-1 if i < 2 else (i - 2) // 3 for i in range(min(n, 26)))}  # two roots, fan-out 3, three levels


def _trees(route, tree):
    """The parents of every sequence of a route's set under a named tree (deep26: 26 nodes wherever the set has nodes at all)."""
    return tuple(TREES[tree](26 if tree == "deep26" and s else s) for _, s in SETS[route])


@functools.lru_cache(maxsize=None)
def _raw(route, geom, dtype):
    """The raw K and V of a set's sequences, [1, hk, L, d] each, on the device: made once, shared, never written."""
    d, _, hk = GEOM[route][geom]
    return tuple(tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dtype, 9000 + 16 * i + d, 2.0)) for i, (n, _) in enumerate(SETS[route]))


@functools.lru_cache(maxsize=None)
def _pool(route, geom, dtype):
    """A set's sequences in a pool, each appended with one call: (cache, seqs).  Only ever read afterwards."""
    from lqer_amd import PagedKVCache

    d, _, hk = GEOM[route][geom]
    lens = [n for n, _ in SETS[route]]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens), hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=max(map(pages_of, lens)))
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v) in zip(seqs, _raw(route, geom, dtype)):
        cache.append([s], k, v)
    return cache, seqs


@functools.lru_cache(maxsize=None)
def _q1(route, geom, dtype, i, c):
    """The c query rows of sequence i, [1, h, c, d]."""
    d, h, _ = GEOM[route][geom]
    return F._randn((1, h, c, d), dtype, 500 + 16 * i + c, 3.0).to(DEV)


def _mask(t, parents, dtype):
    """[1, 1, s, t] from the rule, spelled without tree_masks: 0 where row i sees key j - the context below t - s, and of the draft
    node i itself and its ancestors -, the most negative finite value elsewhere."""
    s = len(parents)
    m = torch.full((s, t), torch.finfo(dtype).min, dtype=dtype)
    m[:, :t - s] = 0
    for i in range(s):
        j = i
        while j >= 0:
            m[i, t - s + j] = 0
            j = parents[j]
    return m.view(1, 1, s, t).to(DEV)


def _rows(out, st):
    return out[0].transpose(0, 1).contiguous(), st[0].transpose(0, 1).contiguous()


def _compare(q1, k, v, parents, kernel):
    """The comparator on ONE sequence's raw tensors with the tree as a mask tensor, as rows [c, h, d] and [c, h, 2]."""
    from lqer_amd import attention_flexible

    return _rows(*attention_flexible(q1, k, v, CFG, CFG, q1.shape[3] ** -0.5, kernel=kernel, return_stats=True,
                                     attention_mask=_mask(k.shape[2], parents, q1.dtype)))


@functools.lru_cache(maxsize=None)
def _want(route, geom, dtype, i, parents):
    """The comparator for sequence i of a set under `parents`.  Made once, never written."""
    k, v = _raw(route, geom, dtype)[i]
    return _compare(_q1(route, geom, dtype, i, len(parents)), k, v, parents, KERNEL[route])


def _queries(route, geom, dtype, pick, trees):
    return torch.cat([_q1(route, geom, dtype, i, len(p))[0].transpose(0, 1) for i, p in zip(pick, trees) if p]).contiguous()


def _check(route, geom, dtype, pick, trees, out, st, what=""):
    at = starts_of([len(p) for p in trees])
    for b, (i, p) in enumerate(zip(pick, trees)):
        if not p:
            continue
        want, want_st = _want(route, geom, dtype, i, p)
        got, got_st = out[at[b]:at[b + 1]], st[at[b]:at[b + 1]]
        assert got.shape == want.shape and got_st.shape == want_st.shape
        assert torch.equal(u8(got), u8(want)), f"{what} sequence {i} {SETS[route][i]}: {(got != want).sum().item()} outputs differ"
        assert torch.equal(u8(got_st), u8(want_st)), f"{what} sequence {i} {SETS[route][i]}: row_stats differ"


# ---- 1. bits per sequence, both routes ---------------------------------------------------------------------------------------------
CASES1 = ([("dec", g, dt, t) for g in GEOM["dec"] for dt in DTYPES for t in ("chain", "star", "binary", "tworoots")]
          + [("pre", g, dt, t) for g in GEOM["pre"] for dt in DTYPES for t in ("chain", "star", "binary", "deep26")])


@pytest.mark.parametrize("route, geom, dtype, tree", CASES1, ids=[f"{r}-{g}-{DT_ID[dt]}-{t}" for r, g, dt, t in CASES1])
def test_bits_per_sequence(route, geom, dtype, tree):
    from lqer_amd import attention_flexible_paged_decode_ragged, attention_flexible_paged_ragged, attention_flexible_paged_tree

    cache, seqs = _pool(route, geom, dtype)
    trees = _trees(route, tree)
    pick = tuple(range(len(seqs)))
    q = _queries(route, geom, dtype, pick, trees)
    scale = q.shape[2] ** -0.5
    plan = attention_flexible_paged_tree.plan(cache, seqs, trees)
    assert [p["call"] for p in plan] == [DECODE if route == "dec" else PREFILL] and plan[0]["rows"] == "view"
    out, st = attention_flexible_paged_tree(q, cache, seqs, trees, scale, return_stats=True)
    assert out.shape == q.shape and out.dtype == q.dtype and st.shape == (*q.shape[:2], 2) and st.dtype == torch.float32
    _check(route, geom, dtype, pick, trees, out, st, what=tree)
    assert torch.isfinite(out).all()
    alone = attention_flexible_paged_tree(q, cache, seqs, trees, scale)  # (without the statistics)
    assert torch.equal(u8(alone), u8(out))
    if tree == "chain":  # a chain is the causal rule: the sibling's bytes
        counts = [len(p) for p in trees]
        if route == "dec":
            c_out, c_st = attention_flexible_paged_decode_ragged(q, cache, seqs, counts, scale, causal=True, return_stats=True)
        else:
            c_out, c_st = attention_flexible_paged_ragged(q, cache, seqs, counts, scale, causal=True, return_stats=True, kernel="prefill")
        assert torch.equal(u8(out), u8(c_out)) and torch.equal(u8(st), u8(c_st))
    if route == "dec" and geom == "d48":  # the prefill entry takes small trees too (kernel="prefill"): ITS comparator's bits
        out_p, st_p = attention_flexible_paged_tree(q, cache, seqs, trees, scale, return_stats=True, kernel="prefill")
        at = starts_of([len(p) for p in trees])
        for b, p in enumerate(trees):
            if p:
                k, v = _raw(route, geom, dtype)[b]
                want, want_st = _compare(_q1(route, geom, dtype, b, len(p)), k, v, p, "prefill")
                assert torch.equal(u8(out_p[at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(st_p[at[b]:at[b + 1]]), u8(want_st)), (tree, b)


@pytest.mark.parametrize("route", ["dec", "pre"])
def test_a_nibble_pool_gives_the_byte_pools_bits(route):
    """K and V formats of width 4 in a code_bits=4 pool and in a byte pool: the same bits, and the comparator's."""
    import test_gpu_kv_nibble as N
    from lqer_amd import PagedKVCache, attention_flexible, attention_flexible_paged_tree

    dt, (d, h, hk) = F16, GEOM[route]["d48"]
    cfg0, cfg1 = N.kv_cfgs(("e4", 4), ("e4", 4))
    sets = SETS[route][:5]
    trees = [TREES["binary"](s) for _, s in sets]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dt, 9500 + i, 2.0)) for i, (n, _) in enumerate(sets)]
    qs = [F._randn((1, h, len(p), d), dt, 640 + i, 3.0).to(DEV) for i, p in enumerate(trees)]
    q = torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous()
    got = []
    for bits in (None, 4):
        cache = PagedKVCache(sum(pages_of(n) for n, _ in sets), len(sets), hk, d, cfg0, cfg1, dt, DEV, max_pages_per_seq=max(pages_of(n) for n, _ in sets),
                             code_bits=bits)
        seqs = [cache.alloc() for _ in sets]
        for s, (k, v) in zip(seqs, raws):
            cache.append([s], k, v)
        got.append(attention_flexible_paged_tree(q, cache, seqs, trees, d ** -0.5, return_stats=True))
    assert torch.equal(u8(got[0][0]), u8(got[1][0])) and torch.equal(u8(got[0][1]), u8(got[1][1]))
    at = starts_of([len(p) for p in trees])
    for b, ((k, v), p) in enumerate(zip(raws, trees)):
        want, want_st = _rows(*attention_flexible(qs[b], k, v, cfg0, cfg1, d ** -0.5, kernel=KERNEL[route], return_stats=True,
                                                  attention_mask=_mask(k.shape[2], p, dt)))
        assert torch.equal(u8(got[1][0][at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(got[1][1][at[b]:at[b + 1]]), u8(want_st)), b


# ---- 2. kernel="auto": both entries in one call --------------------------------------------------------------------------------------
def test_auto_mixes_both_routes_in_one_call():
    """Counts (1, 8, 9, 64, 0) on sequences of 33, 17, 70, 321 and 40 keys: the first two in ONE decode-tree call, the next two in ONE
    prefill-tree call.  Every sequence gets the bits it gets alone - and the comparator's; in another order the rows are gathered."""
    from lqer_amd import PagedKVCache, attention_flexible_paged_tree

    dt, d, h, hk = F16, 48, 4, 2
    lens, counts = (33, 17, 70, 321, 40), (1, 8, 9, 64, 0)
    trees = [TREES["binary"](c) for c in counts]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, n, d), dt, 9600 + i, 2.0)) for i, n in enumerate(lens)]
    cache = PagedKVCache(sum(map(pages_of, lens)), len(lens), hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=max(map(pages_of, lens)))
    seqs = [cache.alloc() for _ in lens]
    for s, (k, v) in zip(seqs, raws):
        cache.append([s], k, v)
    qs = [F._randn((1, h, c, d), dt, 660 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    for order in ((0, 1, 2, 3, 4), (3, 0, 4, 2, 1)):
        o_seqs, o_trees = [seqs[i] for i in order], [trees[i] for i in order]
        plan = attention_flexible_paged_tree.plan(cache, o_seqs, o_trees)
        rows = "view" if order[0] == 0 else "gathered"
        assert [(p["call"], sorted(order[b] for b in p["seqs"]), p["rows"]) for p in plan] == [(DECODE, [0, 1], rows), (PREFILL, [2, 3], rows)]
        q = torch.cat([qs[i][0].transpose(0, 1) for i in order if counts[i]]).contiguous()
        out, st = attention_flexible_paged_tree(q, cache, o_seqs, o_trees, d ** -0.5, return_stats=True)
        at = starts_of([counts[i] for i in order])
        for b, i in enumerate(order):
            if not counts[i]:
                continue
            qi = qs[i][0].transpose(0, 1).contiguous()
            alone, alone_st = attention_flexible_paged_tree(qi, cache, [seqs[i]], [trees[i]], d ** -0.5, return_stats=True)
            want, want_st = _compare(qs[i], *raws[i], trees[i], "decode" if counts[i] <= 8 else "prefill")
            for x, y in ((alone, alone_st), (want, want_st)):
                assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(x)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(y)), (order, i)
        assert torch.isfinite(out).all()


# ---- the C calls themselves: bounds, buffers and a workspace of the caller's -----------------------------------------------------------
def _words(trees):
    """The rows' words on the device, int64 holding the 64 bits."""
    from lqer_amd import tree_masks

    return torch.tensor([m - (1 << 64) if m >> 63 else m for p in trees for m in tree_masks(p)], dtype=torch.int64).to(DEV)


def _ws_need(entry, cache, n_seqs, h, d, max_s, max_len, total):
    from lqer_amd import _lib

    L = _lib.lib()
    if entry == DECODE:
        return L.lqer_attention_q_decode_paged_ragged_workspace_bytes(total, h, max_len, d)
    return L.lqer_attention_q_paged_ragged_workspace_bytes(n_seqs, h, cache.kv_heads, max_s, max_len, d)


def _c_call(entry, cache, seqs, counts, tree, q, out, st, max_s=None, max_len=None, total=None, ws=None, ws_fill=0xFF):
    """One of the two entries as it stands: every sequence of the call is handed over, a count of 0 included; q / out [rows, h, d]
    views with any token and head stride; tree: int64 [>= total] on the device."""
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
        ws = torch.full((max(_ws_need(entry, cache, len(seqs), h, d, max_s, max_len, total), 16),), ws_fill, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(q.device):
        _lib.check(getattr(L, entry)(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(),
                                     st.data_ptr() if st is not None else None, ops.dtype_code(q), len(seqs), h, cache.kv_heads,
                                     cache._call_starts(counts), max_s, total, d, _pair(q), _pair(out), d ** -0.5, 1,
                                     C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), C.byref(f[3]), ws.data_ptr(), ws.numel(),
                                     ops._stream(q.device), tree.data_ptr()), entry)


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["dec", "pre"])
def test_rows_do_not_depend_on_the_batch_the_bounds_or_the_buffers(route):
    """d 128, heads 16 / 2, the binary tree.  Two sequences of the set - alone, inside the whole batch and inside the reversed batch;
    with max_s tight and at the entry's limit; with max_len tight and at the table's room (other workspace strides, another grid); from
    q / out buffers with spare tokens behind `total`, `total` beyond the rows in use and a padded token stride; with the workspace
    pre-filled with 0xFF and with zeros.  Every setting gives the comparator's bits."""
    geom, dt, entry, limit = "d128", F16, DECODE if route == "dec" else PREFILL, 8 if route == "dec" else 64
    d, h, _ = GEOM[route][geom]
    cache, seqs = _pool(route, geom, dt)
    trees_all = _trees(route, "binary")
    pick_all = list(range(len(seqs)))
    for target in ((0, 4) if route == "dec" else (1, 3)):
        want, want_st = (u8(x) for x in _want(route, geom, dt, target, trees_all[target]))
        for order in ([target], pick_all, pick_all[::-1]):
            trees = [trees_all[i] for i in order]
            cs = [len(p) for p in trees]
            total, at, b = sum(cs), starts_of(cs), order.index(target)
            q = _queries(route, geom, dt, order, trees)
            words = torch.cat([_words(trees), torch.full((5,), -1, dtype=torch.int64, device=DEV)])
            for max_s, max_len in ((None, None), (limit, None), (limit, cache.pt.max_len)):
                for fill in (0xFF, 0x00):
                    _, qv = _padded(total, h, d, dt, 5, 24, 0xFF)
                    qv.copy_(q)
                    obase, ov = _padded(total, h, d, dt, 5, 8, 0x5A)
                    sv = torch.full((total + 5, h, 2), 7.0, dtype=torch.float32, device=DEV)
                    _c_call(entry, cache, [seqs[i] for i in order], cs, words, qv, ov, sv, max_s=max_s, max_len=max_len, total=total + 5, ws_fill=fill)
                    assert torch.equal(u8(ov[at[b]:at[b + 1]]), want) and torch.equal(u8(sv[at[b]:at[b + 1]]), want_st), (target, order, max_s, max_len, fill)
                    assert bool((sv[total:] == 7.0).all())
                    keep = torch.ones_like(obase, dtype=torch.bool)
                    keep.as_strided(ov.shape, ov.stride()).fill_(False)
                    assert bool((u8(obase[keep]) == 0x5A).all())  # the spare tokens and the padding of out keep their bytes


def test_bits_above_a_rows_own_are_ignored():
    """Bits j > i of row i are the causal limit's to refuse: all of them set changes nothing (both entries)."""
    from lqer_amd import tree_masks

    for route, entry, i in (("dec", DECODE, 1), ("pre", PREFILL, 2)):
        geom, dt = "d48", F16
        d, h, _ = GEOM[route][geom]
        cache, seqs = _pool(route, geom, dt)
        p = _trees(route, "binary")[i]
        q = _queries(route, geom, dt, [i], [p])
        noisy = torch.tensor([(m | (-1 << (r + 1))) for r, m in enumerate(tree_masks(p))], dtype=torch.int64).to(DEV)
        out = torch.empty_like(q)
        st = torch.empty(len(p), h, 2, dtype=torch.float32, device=DEV)
        _c_call(entry, cache, [seqs[i]], [len(p)], noisy, q, out, st)
        want, want_st = _want(route, geom, dt, i, p)
        assert torch.equal(u8(out), u8(want)) and torch.equal(u8(st), u8(want_st)), route


# ---- 4. zero counts, empty sequences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["dec", "pre"])
def test_zero_counts_and_empty_sequences(route):
    """The whole set through the C call, one sequence with S_b = 0: the others' rows are the comparator's and an out filled with a
    pattern keeps it everywhere else.  Every count 0: nothing at all is written.  A sequence of length 0 WITH a count gets zero rows
    and no statistics."""
    from lqer_amd import PagedKVCache

    geom, dt, entry = "d48", F16, DECODE if route == "dec" else PREFILL
    d, h, hk = GEOM[route][geom]
    cache, seqs = _pool(route, geom, dt)
    trees = list(_trees(route, "star"))
    if route == "pre":
        trees[2] = ()  # (the decode set has its sequence of count 0)
    counts = [len(p) for p in trees]
    total, pick = sum(counts), list(range(len(seqs)))
    q = _queries(route, geom, dt, pick, trees)
    obase, ov = _padded(total, h, d, dt, 3, 16, 0x5A)
    sv = torch.full((total + 3, h, 2), 7.0, dtype=torch.float32, device=DEV)
    _c_call(entry, cache, seqs, counts, _words(trees), q, ov, sv, total=total + 3)
    _check(route, geom, dt, pick, trees, ov, sv[:total])
    keep = torch.ones_like(obase, dtype=torch.bool)
    keep.as_strided(ov.shape, ov.stride()).fill_(False)
    assert bool((u8(obase[keep]) == 0x5A).all()) and bool((sv[total:] == 7.0).all())
    obase.view(torch.uint8).fill_(0x5A)
    sv.fill_(7.0)
    _c_call(entry, cache, seqs, [0] * len(seqs), _words(trees), q, ov, sv, max_s=1, total=total)
    torch.cuda.synchronize()
    assert bool((u8(obase) == 0x5A).all()) and bool((sv == 7.0).all())
    # lens[b] = 0 with a count of 2 beside a sequence of 20 keys with 3 nodes
    small = PagedKVCache(2, 2, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=2)
    empty, full = small.alloc(), small.alloc()
    k, v = (x.to(DEV) for x in KV._kv((1, hk, 20, d), dt, 9700, 2.0))
    small.append([full], k, v)
    q2 = F._randn((1, h, 5, d), dt, 77, 3.0).to(DEV)
    out = torch.full((5, h, d), 3.0, dtype=dt, device=DEV)
    st = torch.full((5, h, 2), 7.0, dtype=torch.float32, device=DEV)
    p = (-1, 0, 0)
    _c_call(entry, small, [empty, full], (2, 3), _words([(-1, 0), p]), q2[0].transpose(0, 1).contiguous(), out, st)
    want, want_st = _compare(q2[:, :, 2:], k, v, p, KERNEL[route])
    assert bool((out[:2] == 0).all()) and bool((st[:2] == 7.0).all())
    assert torch.equal(u8(out[2:]), u8(want)) and torch.equal(u8(st[2:]), u8(want_st))


# ---- 5. footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["dec", "pre"])
def test_footprint(route):
    """Pool and workspace start at 0xFF; q and the masks are guarded inputs; out, statistics, workspace, pool and table carry guard
    zones, and the attention writes nothing of the pool, the table, q or the masks."""
    from lqer_amd import PagedKVCache

    entry = DECODE if route == "dec" else PREFILL
    dt, d, h, hk, stride = F16, 48, 4, 2, 5
    cache = PagedKVCache(16, 4, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=0xFF, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(4, stride)
    seqs = [cache.alloc() for _ in range(4)]
    lens, counts = ((41, 35, 18, 5), (1, 8, 0, 5)) if route == "dec" else ((70, 35, 18, 65), (9, 33, 0, 64))
    trees = [TREES["binary"](c) for c in counts]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t, d), dt, 9800 + i, 2.0)) for i, t in enumerate(lens)]
    for s, (k, v) in zip(seqs, raws):
        cache.append([s], k, v)
    total = sum(counts)
    qs = [F._randn((1, h, c, d), dt, 690 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    g_q = _guard.guarded(total * h * d * 2, align=16, name="q").load(torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous())
    g_tree = _guard.guarded(total * 8, align=16, name="tree").load(_words(trees))
    max_len, max_s = 80, max(counts)
    g_ws = _guard.guarded(_ws_need(entry, cache, 4, h, d, max_s, max_len, total), align=16, fill=0xFF, name="workspace")
    g_out = _guard.guarded(total * h * d * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(total * h * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(total, h, d), g_st.view(torch.float32).view(total, h, 2)
    torch.cuda.synchronize()
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    _c_call(entry, cache, seqs, counts, g_tree.payload.view(torch.int64), g_q.view(dt).view(total, h, d), out, st, max_len=max_len, ws=g_ws.payload)
    torch.cuda.synchronize()
    g_ws.check(), g_out.check(), g_st.check(), g_pool.check(), g_tbl.check(), g_q.unchanged(), g_tree.unchanged()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)
    at = starts_of(counts)
    for b, ((k, v), p) in enumerate(zip(raws, trees)):
        if p:
            want, want_st = _compare(qs[b], k, v, p, KERNEL[route])
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st)), b
    assert torch.isfinite(out).all()


# ---- 6. one step, end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [None, 4], ids=["bytes", "nibbles"])
def test_one_speculative_step_end_to_end(bits):
    """Fork a snapshot, append_ragged a binary tree of 8 nodes, attend, accept the path 0 -> 1 -> 3, free the sequence, append those
    three rows of k / v to the snapshot: a following one-token decode on the snapshot has the bits of a sequence that was only ever
    appended the accepted keys."""
    import test_gpu_kv_nibble as N
    from lqer_amd import PagedKVCache, attention_flexible_paged, attention_flexible_paged_tree

    dt, d, h, hk, ctx = F16, 48, 4, 2, 37
    cfgs = N.kv_cfgs(("e4", 4), ("e4", 4)) if bits else (CFG, CFG)
    parents, path = TREES["binary"](8), [0, 1, 3]
    k, v = (x.to(DEV) for x in KV._kv((1, hk, ctx, d), dt, 9900, 2.0))
    tk, tv = (x.to(DEV)[0].transpose(0, 1).contiguous() for x in KV._kv((1, hk, 8, d), dt, 9901, 2.0))  # the tree's keys, [8, hk, d]
    nk, nv = (x.to(DEV) for x in KV._kv((1, hk, 1, d), dt, 9902, 2.0))                                  # the next step's key
    cache = PagedKVCache(16, 4, hk, d, *cfgs, dt, DEV, max_pages_per_seq=4, code_bits=bits)
    seq = cache.alloc()
    cache.append([seq], k, v)
    snap, = cache.fork(seq)
    cache.append_ragged([seq], tk, tv, [8])
    q = F._randn((8, h, d), dt, 700, 3.0).to(DEV)
    out, st = attention_flexible_paged_tree(q, cache, [seq], [parents], d ** -0.5, return_stats=True)
    # the verify step's own bits: the comparator's on the context plus the whole tree
    from lqer_amd import attention_flexible
    full_k, full_v = torch.cat([k, tk.transpose(0, 1)[None]], 2), torch.cat([v, tv.transpose(0, 1)[None]], 2)
    want, want_st = _rows(*attention_flexible(q.transpose(0, 1)[None].contiguous(), full_k, full_v, *cfgs, d ** -0.5, kernel="decode", return_stats=True,
                                              attention_mask=_mask(ctx + 8, parents, dt)))
    assert torch.equal(u8(out), u8(want)) and torch.equal(u8(st), u8(want_st))
    free_before = cache.pages_free
    cache.free(seq)
    assert cache.pages_free > free_before
    cache.append_ragged([snap], tk[path].contiguous(), tv[path].contiguous(), [3])
    # ... against a sequence that only ever saw the context and the accepted keys
    ref = cache.alloc()
    cache.append([ref], torch.cat([k, tk[path].transpose(0, 1)[None]], 2), torch.cat([v, tv[path].transpose(0, 1)[None]], 2))
    assert cache.length(snap) == cache.length(ref) == ctx + 3
    cache.append([snap, ref], torch.cat([nk, nk]), torch.cat([nv, nv]))
    q1 = F._randn((1, h, 1, d), dt, 701, 3.0).to(DEV)
    got, got_st = attention_flexible_paged(torch.cat([q1, q1]), cache, [snap, ref], d ** -0.5, causal=True, return_stats=True)
    assert torch.equal(u8(got[0]), u8(got[1])) and torch.equal(u8(got_st[0]), u8(got_st[1]))
    raw_k = torch.cat([k, tk[path].transpose(0, 1)[None], nk], 2)
    raw_v = torch.cat([v, tv[path].transpose(0, 1)[None], nv], 2)
    want1, want1_st = attention_flexible(q1, raw_k, raw_v, *cfgs, d ** -0.5, kernel="decode", causal=True, return_stats=True)
    assert torch.equal(u8(got[:1]), u8(want1)) and torch.equal(u8(got_st[:1]), u8(want1_st))

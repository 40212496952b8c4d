"""The prefill kernel that reads the paged pool's codes in its key loop, on the GPU (lqer_attention_q_paged_direct: k_attn_q_direct
of csrc/attn_q.hip; attention_flexible_paged_ragged / attention_flexible_paged_tree with kernel="direct").

The contract is the image route's, an equality of bits per sequence: the rows of sequence b in out and row_stats are those of ONE
batch-1 attention_flexible(q_b, K_b, V_b, ..., kernel="prefill", attention_mask=M) on the sequence's raw K and V - never the paged
code - with M the causal rule, the window or the tree as a tensor of 0 / finfo.min.  The root is the CPU comparator evaluated in fp64.

Causal set (keys, rows): (64, 64) one full tile, base 0; (70, 9) rows over the 64-key tile, the last tile 6 keys and zeros; (100, 33)
one row in the second wave, the subtile at 96; (321, 130) two query tiles, key 320 alone in its tile and on its page; (17, 3) a count
<= 8 on this kernel, the page edge at 16; (40, 0) left out.  Tree set: test_gpu_kv_tree's prefill set and trees.  Window: W = 40,
R = 64, 300 keys, 33 rows (first key seen 228 - page 14 of tile 192: zeros at keys 192 .. 223 inside the first tile) and W = 64, 9 rows
at 200 keys (first key seen 128: the sweeps start at tile 2, the pages below are released)."""
import ctypes as C

import pytest
import torch

import _guard
import test_gpu_kv_tree as T
from _attention import BAR, _rel, comparator
from test_gpu_kv_paged import pages_of, u8
from test_gpu_kv_ragged import _padded, starts_of

pytestmark = pytest.mark.gpu

CFG, DEV, DTYPES, DT_ID, F16, KV, F = T.CFG, T.DEV, T.DTYPES, T.DT_ID, T.F16, T.KV, T.F
DIRECT = "lqer_attention_q_paged_direct"
# the causal set as one more route of test_gpu_kv_tree's tables: its pool, raw tensors, queries and comparator (a chain IS the causal mask)
T.SETS["dir"] = ((64, 64), (70, 9), (100, 33), (321, 130), (17, 3), (40, 0))
T.GEOM["dir"], T.KERNEL["dir"] = T.GEOM["pre"], "prefill"
CHAIN = tuple(T.TREES["chain"](s) for _, s in T.SETS["dir"])
RULES = ("causal", "chain", "star", "binary", "deep26")


def _run(rule, geom, dtype, stats=True):
    """One kernel="direct" call over a whole set: (route, the sequences' parents, out, row_stats)."""
    from lqer_amd import attention_flexible_paged_ragged, attention_flexible_paged_tree

    route = "dir" if rule == "causal" else "pre"
    trees = CHAIN if rule == "causal" else T._trees("pre", rule)
    cache, seqs = T._pool(route, geom, dtype)
    q = T._queries(route, geom, dtype, range(len(seqs)), trees)
    scale = q.shape[2] ** -0.5
    if rule == "causal":
        plan = attention_flexible_paged_ragged.plan(cache, seqs, [len(p) for p in trees], "direct")
        got = attention_flexible_paged_ragged(q, cache, seqs, [len(p) for p in trees], scale, causal=True, return_stats=stats, kernel="direct")
    else:
        plan = attention_flexible_paged_tree.plan(cache, seqs, trees, "direct")
        got = attention_flexible_paged_tree(q, cache, seqs, trees, scale, return_stats=stats, kernel="direct")
    assert [(p["call"], p["rows"]) for p in plan] == [(DIRECT, "view")]
    return (route, trees, *got) if stats else got


# ---- 1. the root: the CPU comparator in fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["causal", "deep26"])
@pytest.mark.parametrize("geom, dtype", [("d48", F16), ("d128", torch.bfloat16), ("d16", torch.float32)], ids=["d48-f16", "d128-bf16", "d16-f32"])
def test_root_is_the_cpu_comparator(rule, geom, dtype):
    """Relative error against comparator(..., acc=float64) per sequence, on the raw K and V with the rule as a mask tensor, under BAR =
    1e-3.  The comparator's own fp32-vs-fp64 spread on these inputs (the worst sequence of a set, measured on the CPU) is 6.7e-8
    (causal) / 1.7e-5 (deep26) for d48 f16, 3.3e-5 / 4.4e-5 for d128 bf16 and 3.4e-7 / 1.0e-7 for d16 f32: a twentieth of the bar at most."""
    route, trees, out, _ = _run(rule, geom, dtype)
    at = starts_of([len(p) for p in trees])
    for i, p in enumerate(trees):
        if not p:
            continue
        k, v = (x.cpu() for x in T._raw(route, geom, dtype)[i])
        q1 = T._q1(route, geom, dtype, i, len(p)).cpu()
        want = comparator(q1, k, v, q1.shape[3] ** -0.5, T._mask(k.shape[2], p, dtype).cpu(), acc=torch.float64)[0]
        err = _rel(out[at[i]:at[i + 1]].cpu(), want[0].transpose(0, 1))
        print(f"{rule} {geom} {DT_ID[dtype]} sequence {T.SETS[route][i]}: rel {err:.3e}")
        assert err <= BAR, (i, err)


# ---- 2. bits per sequence -------------------------------------------------------------------------------------------------------------
CASES = [(r, g, dt) for r in RULES for g in T.GEOM["pre"] for dt in DTYPES]


@pytest.mark.parametrize("rule, geom, dtype", CASES, ids=[f"{r}-{g}-{DT_ID[dt]}" for r, g, dt in CASES])
def test_bits_per_sequence(rule, geom, dtype):
    from lqer_amd import attention_flexible_paged_ragged

    route, trees, out, st = _run(rule, geom, dtype)
    assert st.shape == (*out.shape[:2], 2) and st.dtype == torch.float32
    T._check(route, geom, dtype, range(len(trees)), trees, out, st, what=rule)
    assert torch.isfinite(out).all()
    assert torch.equal(u8(_run(rule, geom, dtype, stats=False)), u8(out))  # (without the statistics)
    if rule == "chain":  # a chain is the causal rule: this kernel's causal call, byte for byte
        cache, seqs = T._pool("pre", geom, dtype)
        q = T._queries("pre", geom, dtype, range(len(seqs)), trees)
        c_out, c_st = attention_flexible_paged_ragged(q, cache, seqs, [len(p) for p in trees], q.shape[2] ** -0.5, causal=True, return_stats=True,
                                                      kernel="direct")
        assert torch.equal(u8(out), u8(c_out)) and torch.equal(u8(st), u8(c_st))


def _window_mask(t, s, w, dtype):
    p, j = torch.arange(s).view(s, 1) + (t - s), torch.arange(t).view(1, t)
    m = torch.zeros(s, t, dtype=dtype)
    m[~((j <= p) & (j > p - w))] = torch.finfo(dtype).min
    return m.view(1, 1, s, t).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=list(DT_ID.values()))
@pytest.mark.parametrize("geom", list(T.GEOM["pre"]))
def test_window_bits_after_release(geom, dtype):
    """Two caches under a window with released pages, one call each: W = 40, R = 64, 300 keys and 33 rows; W = 64, R = 64, 200 keys and
    9 rows.  The table lives in a guarded buffer and every entry beyond the pages held and below the released ones is an out-of-range
    page number: a kernel that followed one would not return the comparator's bits."""
    from lqer_amd import PagedKVCache, attention_flexible, attention_flexible_paged_ragged

    d, h, hk = T.GEOM["pre"][geom]
    for n, (w, rows, t, s) in enumerate(((40, 64, 300, 33), (64, 64, 200, 9))):
        cache = PagedKVCache(pages_of(t), 2, hk, d, CFG, CFG, dtype, DEV, max_pages_per_seq=24, window=w, max_query_rows=rows)
        g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=0, name="block table")
        cache.table = g_tbl.payload.view(torch.int32).view(2, 24)
        k, v = (x.to(DEV) for x in KV._kv((1, hk, t, d), dtype, 9300 + n + d, 2.0))
        seq = cache.alloc()
        for at in range(0, t, 60):
            cache.append([seq], k[:, :, at:at + 60], v[:, :, at:at + 60])
        slot = cache.pt.slot(seq)
        gone, held = cache.pt.released[slot], cache.pt.pages_of[slot]
        lo = t - s - w + 1
        assert 0 < gone <= lo // 16 and held == pages_of(t) and (n or (lo // 16) % 4)  # pages went back; case 0: the first live page is inside a tile
        cache.table[slot, :gone] = cache.pt.num_pages + 1
        cache.table[slot, held:] = cache.pt.num_pages + 1
        cache.table[1 - slot] = cache.pt.num_pages + 1
        q1 = F._randn((1, h, s, d), dtype, 930 + n, 3.0).to(DEV)
        q = q1[0].transpose(0, 1).contiguous()
        plan = attention_flexible_paged_ragged.plan(cache, [seq], [s], "direct")
        assert [(p["call"], p["window"]) for p in plan] == [(DIRECT, w)]
        out, st = attention_flexible_paged_ragged(q, cache, [seq], [s], d ** -0.5, causal=True, return_stats=True, kernel="direct")
        want, want_st = T._rows(*attention_flexible(q1, k, v, CFG, CFG, d ** -0.5, kernel="prefill", return_stats=True,
                                                    attention_mask=_window_mask(t, s, w, dtype)))
        torch.cuda.synchronize()
        g_tbl.check()
        assert torch.equal(u8(out), u8(want)) and torch.equal(u8(st), u8(want_st)), (w, t, s)
        assert torch.isfinite(out).all()


# ---- 3. independence and footprint: the C call itself -----------------------------------------------------------------------------------
def _c_direct(cache, seqs, counts, q, out, st, tree=None, window=0, max_s=None, max_len=None, total=None, ws=None):
    """lqer_attention_q_paged_direct as it stands: every sequence handed over, a count of 0 included; ws: None -> NULL and 0 bytes."""
    from lqer_amd import _lib, ops
    from lqer_amd.kvcache import _pair

    L, f = _lib.lib(), cache.fmts
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[s] for s in slots]
    h, d = q.shape[1], q.shape[2]
    max_len = min((max(lens) + 127) // 128 * 128, cache.pt.max_len) if max_len is None else max_len
    with torch.cuda.device(q.device):
        _lib.check(L.lqer_attention_q_paged_direct(q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(),
                                                   st.data_ptr(), ops.dtype_code(q), len(seqs), h, cache.kv_heads, cache._call_starts(counts),
                                                   max(counts) if max_s is None else max_s, sum(counts) if total is None else total, d, _pair(q),
                                                   _pair(out), d ** -0.5, 1, C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), C.byref(f[3]),
                                                   None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), ops._stream(q.device),
                                                   window, None if tree is None else tree.data_ptr()), DIRECT)


@pytest.mark.parametrize("rule", ["causal", "binary"])
def test_rows_do_not_depend_on_the_batch_the_bounds_or_the_buffers(rule):
    """d 128, heads 16 / 2.  Two sequences of the set - alone, inside the whole batch and inside the reversed batch; max_s tight and at
    a limit (64 with a tree, 4096 without), max_len tight and at the table's room; q / out with spare tokens behind `total`, `total`
    beyond the rows in use and a padded token stride; the workspace NULL.  Every setting gives the comparator's bits."""
    geom, dt = "d128", F16
    route = "dir" if rule == "causal" else "pre"
    d, h, _ = T.GEOM[route][geom]
    cache, seqs = T._pool(route, geom, dt)
    trees_all = CHAIN if rule == "causal" else T._trees("pre", rule)
    pick_all = list(range(len(seqs)))
    for target in (1, 3):
        want, want_st = (u8(x) for x in T._want(route, geom, dt, target, trees_all[target]))
        for order in ([target], pick_all, pick_all[::-1]):
            trees = [trees_all[i] for i in order]
            cs = [len(p) for p in trees]
            total, at, b = sum(cs), starts_of(cs), order.index(target)
            q = T._queries(route, geom, dt, order, trees)
            words = None if rule == "causal" else torch.cat([T._words(trees), torch.full((5,), -1, dtype=torch.int64, device=DEV)])
            limit = 4096 if rule == "causal" else 64
            for max_s, max_len in ((None, None), (limit, None), (limit, cache.pt.max_len)):
                _, qv = _padded(total, h, d, dt, 5, 24, 0xFF)
                qv.copy_(q)
                obase, ov = _padded(total, h, d, dt, 5, 8, 0x5A)
                sv = torch.full((total + 5, h, 2), 7.0, dtype=torch.float32, device=DEV)
                _c_direct(cache, [seqs[i] for i in order], cs, qv, ov, sv, tree=words, max_s=max_s, max_len=max_len, total=total + 5)
                assert torch.equal(u8(ov[at[b]:at[b + 1]]), want) and torch.equal(u8(sv[at[b]:at[b + 1]]), want_st), (target, order, max_s, max_len)
                assert bool((sv[total:] == 7.0).all())
                keep = torch.ones_like(obase, dtype=torch.bool)
                keep.as_strided(ov.shape, ov.stride()).fill_(False)
                assert bool((u8(obase[keep]) == 0x5A).all())  # the spare tokens and the padding of out keep their bytes


def test_footprint():
    """test_gpu_kv_tree's footprint case on this entry: the pool starts at 0xFF; q and the masks are guarded inputs; out, statistics,
    pool and table carry guard zones; the workspace is NULL.  The attention writes nothing of the pool, the table, q or the masks."""
    from lqer_amd import PagedKVCache

    dt, d, h, hk, stride = F16, 48, 4, 2, 5
    cache = PagedKVCache(16, 4, hk, d, CFG, CFG, dt, DEV, max_pages_per_seq=stride)
    g_pool = _guard.guarded(cache.buf.numel(), align=16, fill=0xFF, name="KV pool")
    g_tbl = _guard.guarded(cache.table.numel() * 4, align=16, fill=2, name="block table")
    cache.buf, cache.table = g_pool.payload, g_tbl.payload.view(torch.int32).view(4, stride)
    seqs = [cache.alloc() for _ in range(4)]
    lens, counts = (70, 35, 18, 65), (9, 33, 0, 64)
    trees = [T.TREES["binary"](c) for c in counts]
    raws = [tuple(x.to(DEV) for x in KV._kv((1, hk, t, d), dt, 9800 + i, 2.0)) for i, t in enumerate(lens)]
    for s, (k, v) in zip(seqs, raws):
        cache.append([s], k, v)
    total = sum(counts)
    qs = [F._randn((1, h, c, d), dt, 690 + i, 3.0).to(DEV) for i, c in enumerate(counts)]
    g_q = _guard.guarded(total * h * d * 2, align=16, name="q").load(torch.cat([x[0].transpose(0, 1) for x in qs]).contiguous())
    g_tree = _guard.guarded(total * 8, align=16, name="tree").load(T._words(trees))
    g_out = _guard.guarded(total * h * d * 2, align=16, fill=0xFF, name="out")
    g_st = _guard.guarded(total * h * 2 * 4, align=16, fill=0xFF, name="row_stats")
    out, st = g_out.view(dt).view(total, h, d), g_st.view(torch.float32).view(total, h, 2)
    torch.cuda.synchronize()
    pool_before, tbl_before = g_pool.payload.clone(), g_tbl.payload.clone()
    _c_direct(cache, seqs, counts, g_q.view(dt).view(total, h, d), out, st, tree=g_tree.payload.view(torch.int64), max_len=80)
    torch.cuda.synchronize()
    g_out.check(), g_st.check(), g_pool.check(), g_tbl.check(), g_q.unchanged(), g_tree.unchanged()
    assert torch.equal(g_pool.payload, pool_before) and torch.equal(g_tbl.payload, tbl_before)
    at = starts_of(counts)
    for b, ((k, v), p) in enumerate(zip(raws, trees)):
        if p:
            want, want_st = T._compare(qs[b], k, v, p, "prefill")
            assert torch.equal(u8(out[at[b]:at[b + 1]]), u8(want)) and torch.equal(u8(st[at[b]:at[b + 1]]), u8(want_st)), b
    assert torch.isfinite(out).all()

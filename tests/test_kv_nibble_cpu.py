"""Nibble code storage of the paged KV pool (LQER_Q_MXINT_C4 as k_fmt / v_fmt: include/lqer_hip.h "paged KV pool", nibble codes;
csrc/kv_pack.h; lqer_amd.kvcache.PagedKVCache(code_bits=...)), the part that needs no GPU: the three exports are declared, exported and
bound, the format-aware pool size is the header's formula, every refusal - the library's and Python's - comes before anything touches a
device, and the host layer names the calls of a byte pool."""
import ctypes as C
import os
import re

import pytest
import torch

import _formats as F
from lqer_amd import PagedKVCache, _lib, attention_flexible_paged_ragged, kvcache, ops
from lqer_amd._lib import QFmt
from test_kv_paged_call_cpu import _names
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = _lib.SIGNATURES
NEW = ("lqer_kv_pool_bytes_fmt", "lqer_kv_pool_gather_fmt", "lqer_kv_pool_fork_fmt")
C4, MX = 6, _lib.Q_MXINT


def fmt(kind=MX, width=4, block=16, ew=4, eb=7):
    return QFmt(kind, width, block, ew, eb)


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NEW:
        assert name in SIG
        assert re.search(r"\b(int|size_t) %s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # additive exports
    assert "#define LQER_Q_MXINT_C4 6" in hdr and _lib.Q_MXINT_C4 == C4
    qp = C.POINTER(QFmt)
    # the entries without formats, with the two formats behind their lists (in front of the stream)
    assert SIG["lqer_kv_pool_bytes_fmt"] == (C.c_size_t, SIG["lqer_kv_pool_bytes"][1] + [qp, qp])
    for base in ("lqer_kv_pool_gather", "lqer_kv_pool_fork"):
        assert SIG[base + "_fmt"] == (C.c_int, SIG[base][1][:-1] + [qp, qp] + SIG[base][1][-1:])
        assert _names(base + "_fmt") == _names(base)[:-1] + ["k_fmt", "v_fmt", "stream"]


# ---- the size -------------------------------------------------------------------------------------------------------------------------
def _formula(dtype, pages, slots, kv, d, k4, v4):
    """The header's layout restated: five sections, each rounded up to 256 bytes; a code row is D bytes, or D / 2 with nibbles."""
    up = lambda v: (v + 255) // 256 * 256
    items, esz = pages * kv, 4 if dtype == _lib.F32 else 2
    return (up(items * 16 * (d // 2 if k4 else d)) + up(items * d) + up(items * 16 * (d // 2 if v4 else d)) + up(items * d)
            + up(slots * kv * 16 * d * esz))


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F16, _lib.BF16])
@pytest.mark.parametrize("d", [16, 48, 128])
def test_pool_bytes_fmt_is_the_formula(dtype, d):
    L = _lib.lib()
    for pages, slots, kv in ((1, 1, 1), (7, 3, 2), (1000, 9, 8)):
        shape = (dtype, pages, slots, kv, d)
        plain = L.lqer_kv_pool_bytes(*shape)
        assert plain == _formula(*shape, False, False)
        for kk, vk in ((MX, MX), (C4, C4), (C4, MX), (MX, C4)):
            got = L.lqer_kv_pool_bytes_fmt(*shape, C.byref(fmt(kk)), C.byref(fmt(vk, width=3)))
            assert got == _formula(*shape, kk == C4, vk == C4), (shape, kk, vk)
            # (one item of D = 16 rounds up to the same 256 bytes either way; from the second shape on nibbles are smaller)
            assert got == plain if kk == vk == MX else (got <= plain and (got < plain or pages == 1))
        # a wide operand beside a nibble one: K8V4
        assert L.lqer_kv_pool_bytes_fmt(*shape, C.byref(fmt(MX, width=8)), C.byref(fmt(C4))) == _formula(*shape, False, True)
    # per token and kv head at D = 128: 272 B -> 144 B of codes and exponents
    big = (dtype, 1 << 16, 1, 1, 128)
    stage = 16 * 128 * (4 if dtype == _lib.F32 else 2)
    assert (L.lqer_kv_pool_bytes(*big) - stage) / (16 << 16) == 272
    assert (L.lqer_kv_pool_bytes_fmt(*big, C.byref(fmt(C4)), C.byref(fmt(C4))) - stage) / (16 << 16) == 144


@pytest.mark.parametrize("case, k, v", [
    ("width 8 as nibbles", fmt(C4, width=8), fmt()),
    ("width 5 as nibbles (V)", fmt(), fmt(C4, width=5)),
    ("width 1", fmt(C4, width=1), fmt()),
    ("block 32 as nibbles", fmt(C4, block=32), fmt()),
    ("block 32", fmt(), fmt(block=32)),
    ("a minifloat", QFmt(_lib.Q_MINIFLOAT, 4, -1, 2, 1), fmt()),
    ("the int8 route's kind", fmt(_lib.Q_MXINT_I8), fmt()),
    ("an unknown kind", fmt(7), fmt()),
    ("width 9", fmt(width=9), fmt()),
])
def test_pool_bytes_fmt_is_0_for_what_the_pool_does_not_take(case, k, v):
    L = _lib.lib()
    assert L.lqer_kv_pool_bytes_fmt(_lib.F16, 8, 4, 2, 64, C.byref(k), C.byref(v)) == 0, case
    assert L.lqer_kv_pool_bytes_fmt(_lib.F16, 8, 4, 2, 64, C.byref(v), C.byref(k)) == 0, case


def test_pool_bytes_fmt_is_0_for_what_pool_bytes_refuses():
    L = _lib.lib()
    f = C.byref(fmt(C4))
    assert L.lqer_kv_pool_bytes_fmt(_lib.F16, 8, 4, 2, 64, None, f) == 0 and L.lqer_kv_pool_bytes_fmt(_lib.F16, 8, 4, 2, 64, f, None) == 0
    for shape in ((7, 8, 4, 2, 64), (_lib.F16, 0, 4, 2, 64), (_lib.F16, 8, 0, 2, 64), (_lib.F16, 8, 4, 0, 64), (_lib.F16, 8, 4, 2, 24),
                  (_lib.F16, 8, 4, 2, 144)):
        assert L.lqer_kv_pool_bytes(*shape) == 0 == L.lqer_kv_pool_bytes_fmt(*shape, f, f), shape


# ---- the library's refusals: host-side checks in front of any launch, on pointers that are never dereferenced ---------------------------
POOL_ENTRIES = ["lqer_kv_pool_append", "lqer_kv_pool_append_ragged", "lqer_attention_q_decode_paged", "lqer_attention_q_decode_paged_window",
                "lqer_attention_q_decode_paged_ragged", "lqer_attention_q_paged", "lqer_attention_q_paged_window", "lqer_attention_q_paged_ragged",
                "lqer_attention_q_paged_ragged_window", "lqer_kv_pool_gather_fmt", "lqer_kv_pool_fork_fmt"]
SHARED = "lqer_attention_q_decode_paged_shared"
DENSE_ENTRIES = ["lqer_kv_cache_append", "lqer_kv_cache_unpack", "lqer_attention_q_decode_kv", "lqer_attention_q_kv"]
SHAPE = dict(dtype=_lib.F16, pages=8, slots=4, kv_heads=4, D=64)


def _call(entry, **over):
    """`entry` with an argument per parameter name of its declaration in the header: a valid call on made-up device addresses, but for
    what `over` replaces."""
    st = (C.c_int64 * 3)(4 * 64, 64, 64)
    args = dict(q=0x10000, pool=0x100000, pool_bytes=1 << 24, block_table=0x200000, table_stride=4, seq_slots=0x300000, lens=0x400000, max_len=64,
                out=0x40000, row_stats=None, batch=3, heads=4, S=1, q_strides=st, out_strides=st, k_strides=st, v_strides=st, mask_strides=st,
                scaling=0.125, causal=1, q_fmt=fmt(width=8), k_fmt=fmt(), p_fmt=fmt(width=8), v_fmt=fmt(), workspace=0x50000,
                workspace_bytes=1 << 26, stream=None, window=16, q_starts=0x500000, new_starts=0x500000, max_s=1, max_n=1, total=3, k_new=0x600000,
                v_new=0x700000, n=1, len=0, grp_of=0x500100, grp_starts=0x500200, grp_members=0x500300, grp_keys=0x500400, n_groups=2, slot=0, T=16,
                cache=0x800000, cache_bytes=1 << 24, capacity=16, src_slots=0x900000, dst_slots=0x900100, mask=None, k_f32=0xA00000, v_f32=0xB00000,
                **SHAPE)
    args.update(over)
    vals = [C.byref(args[n]) if isinstance(args[n], QFmt) else args[n] for n in _names(entry)]
    L = _lib.lib()
    return getattr(L, entry)(*vals), L.lqer_last_error().decode()


def _who(entry):
    return entry[len("lqer_"):] + ":"


@pytest.mark.parametrize("entry", POOL_ENTRIES)
def test_every_pool_entry_refuses_a_nibble_kind_it_cannot_store(entry):
    for case, over in (("width 8", dict(k_fmt=fmt(C4, width=8))), ("width 5 (V)", dict(v_fmt=fmt(C4, width=5))),
                       ("block 32", dict(k_fmt=fmt(C4, block=32))), ("block 32 (V)", dict(v_fmt=fmt(C4, block=32)))):
        rc, msg = _call(entry, **over)
        assert rc == E_UNSUPPORTED and msg.startswith(_who(entry)) and "LQER_Q_MXINT_C4" in msg, (case, rc, msg)


@pytest.mark.parametrize("entry", POOL_ENTRIES)
@pytest.mark.parametrize("kinds", [(C4, C4), (C4, MX), (MX, C4)], ids=["K4V4", "K4V8", "K8V4"])
def test_a_pool_one_byte_short_of_the_format_aware_size(entry, kinds):
    """The check sizes the pool by the formats: one byte short of lqer_kv_pool_bytes_fmt is refused, and the refusal names that function;
    the byte pool's size would have passed."""
    L = _lib.lib()
    k, v = fmt(kinds[0]), fmt(kinds[1], width=8 if kinds[1] == MX else 3)
    shape = tuple(SHAPE[n] for n in ("dtype", "pages", "slots", "kv_heads", "D"))
    need = L.lqer_kv_pool_bytes_fmt(*shape, C.byref(k), C.byref(v))
    assert 0 < need < L.lqer_kv_pool_bytes(*shape)
    rc, msg = _call(entry, k_fmt=k, v_fmt=v, pool_bytes=need - 1)
    assert rc == E_INVALID and msg.startswith(_who(entry)) and f"{need - 1} B < {need} B (lqer_kv_pool_bytes_fmt)" in msg, (rc, msg)


@pytest.mark.parametrize("entry", [e for e in POOL_ENTRIES if "attention" in e] + [SHARED])
def test_the_kind_is_no_q_or_p_format(entry):
    for name in ("q_fmt", "p_fmt"):
        rc, msg = _call(entry, **{name: fmt(C4)})
        assert rc == E_UNSUPPORTED and "LQER_Q_MXINT_C4" in msg, (name, rc, msg)


@pytest.mark.parametrize("entry", DENSE_ENTRIES)
def test_the_dense_cache_refuses_the_kind(entry):
    for name in ("k_fmt", "v_fmt"):
        rc, msg = _call(entry, **{name: fmt(C4)})
        assert rc == E_UNSUPPORTED and "LQER_Q_MXINT_C4" in msg and "paged KV pool" in msg, (name, rc, msg)


def test_the_grouped_entry_refuses_the_kind():
    for over in (dict(k_fmt=fmt(C4)), dict(v_fmt=fmt(C4)), dict(k_fmt=fmt(C4), v_fmt=fmt(C4, width=2))):
        rc, msg = _call(SHARED, **over)
        assert rc == E_UNSUPPORTED and msg.startswith(_who(SHARED)) and "lqer_attention_q_decode_paged" in msg, (rc, msg)
    rc, msg = _call(SHARED, pool_bytes=1024)  # (with byte codes the entry checks as ever)
    assert rc == E_INVALID and "(lqer_kv_pool_bytes)" in msg


def test_the_entries_without_formats_size_a_byte_pool():
    L = _lib.lib()
    shape = tuple(SHAPE[n] for n in ("dtype", "pages", "slots", "kv_heads", "D"))
    need = L.lqer_kv_pool_bytes(*shape)
    for entry in ("lqer_kv_pool_gather", "lqer_kv_pool_fork"):
        rc, msg = _call(entry, pool_bytes=need - 1)
        assert rc == E_INVALID and f"< {need} B (lqer_kv_pool_bytes)" in msg, (entry, rc, msg)
        rc, msg = _call(entry + "_fmt", pool_bytes=need - 1)  # both kinds LQER_Q_MXINT: the same pool
        assert rc == E_INVALID and f"< {need} B (lqer_kv_pool_bytes)" in msg, (entry, rc, msg)
        rc, msg = _call(entry + "_fmt", k_fmt=None)
        assert rc == E_INVALID, (entry, rc, msg)
        rc, msg = _call(entry + "_fmt", v_fmt=QFmt(_lib.Q_MINIFLOAT, 4, -1, 2, 1))
        assert rc == E_UNSUPPORTED, (entry, rc, msg)


# ---- Python ---------------------------------------------------------------------------------------------------------------------------------
def _cfg(fid, width):
    c = F.cfg(fid, width, [1, 16], True)
    return dict(name="flexible", default=c, x_quantizer=c, w_quantizer=c)


def _host_cache(code_bits, k=("e4", 4), v=("e4", 3), **kw):
    """test_kv_paged_call_cpu's host cache - buffers in host memory, launches that do nothing - with a parent of 37 keys, two forks of it
    and a stranger of 20."""
    x = F.cfg("e8", 8, [1, 16], True)
    cfg0 = dict(name="flexible", default=x, x_quantizer=x, w_quantizer=F.cfg(*k, [1, 16], True))
    cfg1 = dict(name="flexible", default=x, x_quantizer=x, w_quantizer=F.cfg(*v, [1, 16], True))
    cache = PagedKVCache(16, 6, 2, 16, cfg0, cfg1, torch.float16, "cpu", max_pages_per_seq=16, code_bits=code_bits, **kw)
    cache._launch_append = cache._launch_append_ragged = cache._launch_fork = lambda *a: None
    z = lambda n: torch.zeros(1, 2, n, 16, dtype=torch.float16)
    parent, lone = cache.alloc(), cache.alloc()
    cache.append([parent], z(37), z(37))
    cache.append([lone], z(20), z(20))
    kids = cache.fork(parent, 2)
    return cache, [kids[0], lone, parent, kids[1]]


def test_code_bits_none_and_8_are_the_byte_pool():
    L = _lib.lib()
    for bits in (None, 8, (8, 8), (None, 8)):
        cache, _ = _host_cache(bits)
        assert cache.code_bits == (8, 8) and not cache.nibble
        assert cache.nbytes == L.lqer_kv_pool_bytes(_lib.F16, 16, 6, 2, 16)
        assert [f.kind for f in cache.fmts] == [MX] * 4
        assert cache._with_code_fmts("lqer_kv_pool_gather") == ("lqer_kv_pool_gather", ())


@pytest.mark.parametrize("bits, kinds", [(4, (C4, C4)), ((4, 4), (C4, C4)), ((4, 8), (C4, MX)), ((8, 4), (MX, C4)), ((None, 4), (MX, C4))])
def test_code_bits_4_sizes_the_pool_by_the_formats(bits, kinds):
    L = _lib.lib()
    cache, _ = _host_cache(bits)
    assert cache.nibble and cache.code_bits == tuple(4 if k == C4 else 8 for k in kinds)
    assert (cache.fmts[1].kind, cache.fmts[3].kind) == kinds and cache.fmts[0].kind == cache.fmts[2].kind == MX
    assert (cache.fmts[1].width, cache.fmts[3].width) == (4, 3)
    want = L.lqer_kv_pool_bytes_fmt(_lib.F16, 16, 6, 2, 16, C.byref(cache.fmts[1]), C.byref(cache.fmts[3]))
    assert cache.nbytes == cache.buf.numel() == want == _formula(_lib.F16, 16, 6, 2, 16, kinds[0] == C4, kinds[1] == C4)
    assert cache.nbytes < L.lqer_kv_pool_bytes(_lib.F16, 16, 6, 2, 16)
    name, fmts = cache._with_code_fmts("lqer_kv_pool_fork")
    assert name == "lqer_kv_pool_fork_fmt" and len(fmts) == 2


def test_code_bits_4_on_a_wider_config_raises_before_anything_is_allocated(monkeypatch):
    def no_alloc(*a, **k):
        raise AssertionError("allocated")

    monkeypatch.setattr(torch, "empty", no_alloc)
    monkeypatch.setattr(torch, "zeros", no_alloc)
    with pytest.raises(ValueError, match="width 8"):
        PagedKVCache(16, 6, 2, 16, _cfg("e8", 8), _cfg("e8", 8), torch.float16, "cpu", code_bits=4)
    with pytest.raises(ValueError, match="for V.*width 5"):
        PagedKVCache(16, 6, 2, 16, _cfg("e4", 4), _cfg("e4", 5), torch.float16, "cpu", code_bits=(8, 4))
    with pytest.raises(ValueError, match="for K.*width 6"):
        PagedKVCache(16, 6, 2, 16, _cfg("e4", 6), _cfg("e4", 4), torch.float16, "cpu", code_bits=(4, 8))
    for bad in (2, 16, True, "4", (4,), (4, 4, 4), (4, 3), 4.0):
        with pytest.raises((ValueError, TypeError)):
            PagedKVCache(16, 6, 2, 16, _cfg("e4", 4), _cfg("e4", 4), torch.float16, "cpu", code_bits=bad)


def test_nibble_qfmt():
    f = ops.nibble_qfmt(fmt(width=3, ew=3, eb=6))
    assert (f.kind, f.width, f.block, f.exp_width, f.exp_bias) == (C4, 3, 16, 3, 6)
    for bad in (fmt(width=5), fmt(block=32), fmt(_lib.Q_INT), fmt(C4)):
        with pytest.raises(ValueError):
            ops.nibble_qfmt(bad)


def test_plan_names_the_calls_of_a_byte_pool():
    counts = [1, 33, 3, 8]
    plans = []
    for bits in (None, 4, (4, 8)):
        cache, seqs = _host_cache(bits)
        plans.append([attention_flexible_paged_ragged.plan(cache, seqs, counts, kernel=k) for k in ("auto", "prefill")])
    assert plans[0] == plans[1] == plans[2]
    assert [c["call"] for c in plans[1][0]] == [kvcache.RAGGED_DECODE, kvcache.RAGGED_PREFILL]
    plans = []
    for bits in (None, 4):
        cache, seqs = _host_cache(bits, window=24, max_query_rows=40)
        plans.append(attention_flexible_paged_ragged.plan(cache, seqs, [33, 1, 3, 8]))  # (33 rows on 37 keys: beyond the window)
    assert plans[0] == plans[1] and [c["call"] for c in plans[1]] == [kvcache.RAGGED_DECODE, kvcache.RAGGED_PREFILL + "_window"]


@pytest.mark.parametrize("base, window, shape", [
    (kvcache.PAGED_DECODE, None, dict(S=3)), (kvcache.PAGED_DECODE, 16, dict(S=3)), (kvcache.PAGED_PREFILL, None, dict(S=3)),
    (kvcache.PAGED_PREFILL, 16, dict(S=3)), (kvcache.RAGGED_PREFILL, None, dict(counts=[3, 1, 0, 2])),
    (kvcache.RAGGED_PREFILL, 16, dict(counts=[3, 1, 0, 2])), (kvcache.RAGGED_DECODE, None, dict(counts=[3, 1, 0, 2])),
    (kvcache.RAGGED_DECODE, 16, dict(counts=[3, 1, 0, 2]))])
def test_the_builder_names_the_entry_of_a_byte_pool_and_hands_it_the_kinds(base, window, shape):
    got = []
    for bits in (None, 4):
        cache, seqs = _host_cache(bits)
        slots = cache.pt.slots(seqs)
        lens = [cache.pt.lengths[x] for x in slots]
        q = torch.zeros((6, 4, 16) if "counts" in shape else (4, 4, 3, 16), dtype=torch.float16)
        name, args = kvcache._paged_args(base, q, q, None, cache, slots, lens, 0.25, True, window, 0, 0, None, **shape)
        assert len(args) == len(SIG[name][1])
        byname = dict(zip(_names(name), args))
        assert byname["pool_bytes"] == cache.nbytes
        got.append((name, [byname[n]._obj.kind for n in ("q_fmt", "k_fmt", "p_fmt", "v_fmt")]))
    assert got[0][0] == got[1][0]
    assert got[0][1] == [MX] * 4 and got[1][1] == [MX, C4, MX, C4]


def test_shared_prefix_names_the_ungrouped_entry_on_a_nibble_pool():
    chunk_of = lambda t: 16 * min(max((t + 255) // 256, 1), 8)
    for bits, want in ((None, kvcache.SHARED_DECODE), (4, kvcache.PAGED_DECODE), ((8, 4), kvcache.PAGED_DECODE)):
        cache, seqs = _host_cache(bits)
        slots = cache.pt.slots(seqs)
        lens = [cache.pt.lengths[x] for x in slots]
        groups = cache.pt.prefix_groups(slots, lens, chunk_of)
        assert groups == [([0, 2, 3], 32), ([1], 0)]  # the books know the shared pages on either pool
        q = torch.zeros(4, 4, 3, 16, dtype=torch.float16)
        name, args = kvcache._paged_args(kvcache.PAGED_DECODE, q, q, None, cache, slots, lens, 0.25, True, None, 0, 0, None, S=3, groups=groups)
        assert name == want and len(args) == len(SIG[want][1]), bits

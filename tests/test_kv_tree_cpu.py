"""A draft tree per sequence on the paged KV pool (lqer_attention_q_decode_paged_tree, lqer_attention_q_paged_tree: the TREE
instantiations of csrc/attn_decode.hip and csrc/attn_q.hip; tree_masks, attention_flexible_paged_tree), the part that needs no GPU:
the two C-ABI exports are declared, exported and bound and bring no size function of their own, every refusal comes with its code and
a message before anything touches the device, a row's mask follows from the parents, the Python function refuses with the pool's
books as they were, and .plan names the calls from host state alone."""
import ctypes as C
import inspect
import os
import re

import pytest

from lqer_amd import _lib
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, MINIFLOAT, POOL_OK, _fmt, _state
from test_kv_ragged_cpu import _host_cache, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE, PREFILL = "lqer_attention_q_decode_paged_tree", "lqer_attention_q_paged_tree"
HEAP64 = [(i - 1) // 2 for i in range(64)]  # parent = (i - 1) // 2; node 0: -1


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in (DECODE, PREFILL):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
        # the siblings' workspace: no size function of their own, anywhere
        assert name + "_workspace_bytes" not in _lib.SIGNATURES and not re.search(r"\b%s_workspace_bytes\s*\(" % name, hdr)
        assert not hasattr(_lib.lib(), name + "_workspace_bytes")
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    assert "#define LQER_ABI_VERSION 14" in hdr
    rg, dr = _lib.SIGNATURES["lqer_attention_q_paged_ragged"][1], _lib.SIGNATURES["lqer_attention_q_decode_paged_ragged"][1]
    assert dr == rg + [C.c_int64]
    assert _lib.SIGNATURES[DECODE][1] == dr[:-1] + [C.c_void_p]  # the trailing `window` replaced by `tree`
    assert _lib.SIGNATURES[PREFILL][1] == rg + [C.c_void_p]      # ... plus `tree`
    tree_doc = hdr[hdr.index("A DRAFT TREE"):hdr.index("lqer_kv_pool_gather: one sequence")]
    for words in ("SAME BITS", "additive mask", "share blocks of the K quantizer", "bit i of row i is set", "1 <= max_s <= 8", "1 <= max_s <= 64"):
        assert words in tree_doc, words


def _ws_bytes(entry, batch=2, heads=4, kv=4, max_s=8, max_len=64, D=64, total=9):
    L = _lib.lib()
    if entry == DECODE:
        return L.lqer_attention_q_decode_paged_ragged_workspace_bytes(total, heads, max_len, D)
    return L.lqer_attention_q_paged_ragged_workspace_bytes(batch, heads, kv, max_s, max_len, D)


def _attend(entry, q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000,
            max_len=64, out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=2, heads=4, kv=4, starts=0x500000, max_s=8, total=9, D=64, fmts=None,
            causal=1, dtype=_lib.F16, qs=True, os_=True, tree=0x600000):
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = pair(heads * D, D)
    rc = getattr(L, entry)(q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, dtype, batch, heads, kv, starts, max_s,
                           total, D, st if qs else None, st if os_ else None, 0.125, causal,
                           *[C.byref(f) if f != "null" else None for f in fmts], ws, ws_bytes, None, tree)
    return rc, L.lqer_last_error().decode()


# what both entries refuse alike: the additions, then what the siblings refuse
COMMON = [
    ("null tree", dict(tree=None), E_INVALID),
    ("causal = 0", dict(causal=0), E_INVALID),
    ("null q_starts", dict(starts=None), E_INVALID),
    ("max_s = 0", dict(max_s=0), E_INVALID),
    ("negative max_s", dict(max_s=-1), E_INVALID),
    ("negative total", dict(total=-1), E_INVALID),
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("Q width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("K minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), E_UNSUPPORTED),
    ("null format", dict(fmts=[_fmt(), "null", _fmt(), _fmt()]), E_INVALID),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("negative batch", dict(batch=-1), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    ("null q", dict(q=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null q strides", dict(qs=False), E_INVALID),
    ("null out strides", dict(os_=False), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("batch > 65535", dict(batch=65536), E_UNSUPPORTED),
    ("null block_table", dict(tbl=None), E_INVALID),
    ("null seq_slots", dict(seq_slots=None), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("pages = 0", dict(pages=0), E_INVALID),
    ("slots = 0", dict(slots=0), E_INVALID),
    ("table_stride = 0", dict(stride=0), E_INVALID),
    ("max_len = 0", dict(max_len=0), E_INVALID),
    ("max_len > 16 table_stride", dict(max_len=65), E_INVALID),
    ("max_len > 2^30", dict(max_len=(1 << 30) + 1, stride=1 << 27, ws_bytes=1 << 62), E_UNSUPPORTED),
    ("null pool", dict(pool=None), E_INVALID),
    ("pool not 16-byte aligned", dict(pool=0x100008), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
]
OWN = {
    DECODE: [("max_s = 9", dict(max_s=9), E_INVALID), ("max_s = 64", dict(max_s=64), E_INVALID),
             ("short workspace", dict(ws_bytes=_ws_bytes(DECODE) - 1), E_INVALID)],
    PREFILL: [("max_s = 65", dict(max_s=65, total=66), E_INVALID), ("max_s = 300", dict(max_s=300, total=301), E_INVALID),
              ("short workspace", dict(ws_bytes=_ws_bytes(PREFILL) - 1), E_INVALID),
              ("batch x kv_heads > 65535", dict(batch=16384, ws_bytes=1 << 40), E_UNSUPPORTED),
              ("max_len beyond the image grid", dict(max_len=65535 * 64 + 1, stride=1 << 19, ws_bytes=1 << 40), E_UNSUPPORTED)],
}
REFUSALS = [(e, *c) for e in (DECODE, PREFILL) for c in COMMON + OWN[e]]


@pytest.mark.parametrize("entry, case, kwargs, want", REFUSALS, ids=[f"{'decode' if e == DECODE else 'prefill'}-{c}" for e, c, _, _ in REFUSALS])
def test_refusals_before_any_gpu_call(entry, case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _attend(entry, **kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith(entry[len("lqer_"):] + ":"), (case, msg)  # the message names the call
    if case == "null tree":
        assert "tree" in msg, msg
    if case == "causal = 0":
        assert "causal" in msg, msg
    if case.startswith("max_s = ") and kwargs["max_s"] > 8:
        assert "max_s = %d" % kwargs["max_s"] in msg and ("up to 8" if entry == DECODE else "up to 64") in msg, msg
    if case == "short workspace":  # sized by the sibling's function
        assert ("lqer_attention_q_decode_paged_ragged_workspace_bytes" if entry == DECODE else "lqer_attention_q_paged_ragged_workspace_bytes") in msg, msg


@pytest.mark.parametrize("entry", [DECODE, PREFILL])
def test_the_bounds_themselves_pass_the_check_and_nothing_to_do_is_ok(entry):
    assert _attend(entry, batch=0)[0] == 0 and _attend(entry, total=0)[0] == 0
    # max_s at the entry's limit with nothing to do: not refused (8 / 64 are inside)
    assert _attend(entry, max_s=8 if entry == DECODE else 64, total=0)[0] == 0
    assert _attend(entry, max_s=9 if entry == DECODE else 65, total=0)[0] == E_INVALID  # (a bound is judged before the counts are)


def test_tree_masks():
    from lqer_amd import tree_masks

    assert tree_masks([]) == []
    assert tree_masks(range(-1, 63)) == [(2 << i) - 1 for i in range(64)]  # a chain: the causal rule
    assert tree_masks([-1] * 64) == [1 << i for i in range(64)]            # a star: every node sees itself alone
    assert tree_masks([-1, 0, 0, 1, 1, 2, 2, 3]) == [0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100101, 0b1000101, 0b10001011]
    assert tree_masks([-1, -1, 0, 1, 2, 3]) == [0b1, 0b10, 0b101, 0b1010, 0b10101, 0b101010]  # two roots, two chains
    heap = tree_masks(HEAP64)
    assert heap[63] >> 63 == 1 and heap[63] == sum(1 << j for j in (63, 31, 15, 7, 3, 1, 0))  # row 63's own bit is bit 63
    assert all(m >> i == 1 for i, m in enumerate(heap))  # bit i of row i, and no bit above it
    for bad in ([-1] * 65, [0], [-1, 1], [-1, 2, 0], [-2], [-1, 0, -2], ["x"], 7):
        with pytest.raises(ValueError, match="tree_masks"):
            tree_masks(bad)


def _tree_cache(window=None):
    """Three sequences of 70, 8 and 3 keys and an empty one, on the host (test_kv_ragged_cpu's cache: launches do nothing)."""
    import torch

    cache = _host_cache(12, 4, window, max_pages_per_seq=6)
    seqs = [cache.alloc() for _ in range(4)]
    for s, n in zip(seqs, (70, 8, 3)):
        kv = torch.zeros(1, 2, n, 16, dtype=torch.float16)
        cache.append([s], kv, kv)
    return cache, seqs


def test_python_refusals_leave_the_books_alone():
    import torch

    import lqer_amd
    from lqer_amd import attention_flexible_paged_tree

    p = inspect.signature(attention_flexible_paged_tree).parameters
    assert list(p) == ["q", "cache", "seqs", "parents", "scaling", "return_stats", "ws", "kernel"]
    assert p["kernel"].default == "auto" and p["return_stats"].default is False and p["ws"].default is None
    assert callable(lqer_amd.tree_masks) and callable(lqer_amd.attention_flexible_paged_tree)
    cache, (a, b, c, e) = _tree_cache()
    q = lambda n, h=4, d=16, dt=torch.float16: torch.zeros(n, h, d, dtype=dt)
    chain = lambda n: list(range(-1, n - 1))
    before = _state(cache.pt)
    for what, args, kw, match in [
            ("an unknown kernel", (q(2), [a], [chain(2)]), dict(kernel="decode"), "kernel"),
            ("an unknown kernel", (q(2), [a], [chain(2)]), dict(kernel="flash"), "kernel"),
            ("more than 64 nodes", (q(65), [a], [chain(65)]), {}, "64"),
            ("a parent at its node's index", (q(2), [a], [[-1, 1]]), {}, "parent"),
            ("a parent below -1", (q(2), [a], [[-1, -2]]), {}, "parent"),
            ("a parents list too few", (q(2), [a, b], [chain(2)]), {}, "parent lists"),
            ("parents that are no lists", (q(2), [a], [2]), {}, "parents"),
            ("rows that are not the nodes", (q(3), [a], [chain(2)]), {}, "sum\\(counts\\)"),
            ("more nodes than keys", (q(4), [c], [chain(4)]), {}, "query rows <= the length"),
            ("nodes on an empty sequence", (q(1), [e], [[-1]]), {}, "empty sequence"),
            ("an unknown sequence", (q(1), [99], [[-1]]), {}, "99"),
            ("a sequence named twice", (q(2), [a, a], [[-1], [-1]]), {}, "."),
            ("a wrong head dim", (q(2, d=32), [a], [chain(2)]), {}, "cache"),
            ("a wrong dtype", (q(2, dt=torch.bfloat16), [a], [chain(2)]), {}, "cache"),
            ("heads no multiple of kv heads", (q(2, h=3), [a], [chain(2)]), {}, "cache")]:
        with pytest.raises(ValueError, match=match):
            attention_flexible_paged_tree(args[0], cache, args[1], args[2], 0.25, **kw)
        assert _state(cache.pt) == before, what
    windowed, (wa, *_) = _tree_cache(window=16)
    before = _state(windowed.pt)
    for call in (lambda: attention_flexible_paged_tree(q(2), windowed, [wa], [chain(2)], 0.25),
                 lambda: attention_flexible_paged_tree.plan(windowed, [wa], [chain(2)])):
        with pytest.raises(ValueError, match="window"):
            call()
    assert _state(windowed.pt) == before


def test_plan_names_the_calls_from_host_state_alone():
    from lqer_amd import attention_flexible_paged_tree

    cache, _ = _tree_cache()
    chain = lambda n: list(range(-1, n - 1))
    plan = attention_flexible_paged_tree.plan
    seqs = [10, 11, 12, 13, 14]  # (no length is read: the books need not know them)
    trees = [chain(c) for c in (1, 8, 9, 64, 0)]
    assert plan(cache, seqs, trees) == [{"call": DECODE, "seqs": [0, 1], "rows": "view"}, {"call": PREFILL, "seqs": [2, 3], "rows": "view"}]
    assert plan(cache, seqs, trees, kernel="prefill") == [{"call": PREFILL, "seqs": [0, 1, 2, 3], "rows": "view"}]
    mixed = [chain(c) for c in (9, 1, 64, 0, 8)]
    assert plan(cache, seqs, mixed) == [{"call": DECODE, "seqs": [1, 4], "rows": "gathered"}, {"call": PREFILL, "seqs": [0, 2], "rows": "gathered"}]
    assert plan(cache, seqs[:2], [[], []]) == []
    assert plan(cache, [1], [HEAP64]) == [{"call": PREFILL, "seqs": [0], "rows": "view"}]
    for bad, kw in (([chain(65)], {}), ([[-1, 5]], {}), ([chain(2), chain(2)], {}), ([chain(2)], dict(kernel="decode"))):
        with pytest.raises(ValueError):
            plan(cache, [1], bad, **kw)


def test_the_gpu_sets_reach_the_edges_they_are_there_for():
    """Host arithmetic of the kernels' rules for the sets of tests/test_gpu_kv_tree.py (spelled here again: this file imports no GPU test)."""
    from lqer_amd import tree_masks

    chunk = lambda t: 16 * min(max((t + 255) // 256, 1), 8)
    nch = lambda t: -(-t // chunk(t))
    # the decode route: (keys, nodes)
    dec = ((8, 8), (17, 8), (33, 1), (257, 6), (2049, 8))
    assert all(1 <= s <= 8 and s <= t for t, s in dec)
    assert dec[0][0] - dec[0][1] == 0                                             # base 0: no committed context
    assert 17 - 8 == 9 and 9 < 16 <= 16 and chunk(17) == 16 and nch(17) == 2      # draft keys 9 .. 16 straddle the page and chunk edge at 16
    assert chunk(257) == 32 and 257 - 6 == 251 and 251 // 32 == 7 and 256 // 32 == 8  # draft keys 251 .. 256 straddle key 256, chunks 7 and 8
    assert chunk(2049) == 128 and nch(2049) == 17 and 2049 - 8 + 7 == 2048 == 16 * 128  # the last chunk holds draft node 7 alone
    binary = tree_masks([-1, 0, 0, 1, 1, 2, 2, 3])
    assert [i for i, m in enumerate(binary) if not m >> 7 & 1] == list(range(7))  # ... which no row but row 7 sees: a chunk with no visible key
    assert {8 * s for _, s in dec} >= {8, 48, 64} and 8 * 6 > 32 > 8 * 1          # rep 8: rows per kv head on both sides of the 32-row group
    # the prefill route
    pre = ((64, 64), (70, 9), (100, 33), (321, 64))
    assert all(9 <= s <= 64 and s <= t for t, s in pre)
    assert pre[0][0] - pre[0][1] == 0 and tree_masks(HEAP64)[63] >> 63 == 1      # base 0, row 63's bit 63
    assert 70 - 9 == 61 and 61 < 64 <= 69                                         # the smallest count beyond the decode route; keys 61 .. 69 straddle the 64-key tile
    assert 33 > 32 and 100 - 33 == 67 and 67 < 96 <= 99                           # one row in the second wave; the region straddles the 32-key subtile at 96
    assert 321 - 64 == 257 and 320 % 64 == 0 and 321 - 320 == 1                   # key 320 alone in its tile
    deep = [-1, -1] + [i // 3 for i in range(6)] + [2 + i // 3 for i in range(18)]
    depth = [bin(m).count("1") for m in tree_masks(deep)]
    assert len(deep) == 26 and (depth.count(1), depth.count(2), depth.count(3)) == (2, 6, 18)  # two roots, three levels, fan-out 3

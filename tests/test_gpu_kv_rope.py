"""Rotary position embedding inside the paged pool's append, on the GPU (lqer_kv_pool_append_rope: k_kv_rope of csrc/kv_rope.hip;
PagedKVCache.append_ragged_rope).

The comparator is the rule of csrc/kv_rope.hip's header comment evaluated in float64 on the CPU with a cast to the dtype after each of
its three operations - which is eager torch in the dtype: a product of two dtype values is exact in float64, and a sum rounded once
more is correctly rounded.  The pool is compared with a second pool that append_ragged fed the comparator's rotated keys.  Every
comparison is torch.equal on the bytes; there is no tolerance in this file.  Sets and rounds are test_gpu_kv_paged.py's and
test_gpu_kv_ragged.py's (A: D 48 - six runs of 4 on four lanes; B: appends from len % 16 = 15, counts over many blocks) plus G: D 128,
heads 8 / 2, a block closed exactly and one left open behind a closed one."""
import functools

import pytest
import torch

import test_gpu_attention_fused as F
import test_gpu_kv_cache as KV
from _kv_walk import CFG4
from test_gpu_kv_paged import SETS, _raw, _same_live_bytes, pages_of, u8
from test_gpu_kv_ragged import ROUNDS, _packed

pytestmark = pytest.mark.gpu

CFG, DEV = F.CFG, F.DEV
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT_ID = {F16: "f16", BF16: "bf16", F32: "f32"}
ROWS = 640  # of the tables: beyond B's 300 keys + its largest count
GEOMS = {name: (ROUNDS[name], *SETS[name][1:]) for name in "AB"}  # the two rounds' counts, d, heads, kv heads
GEOMS["G"] = (((3, 16, 0), (14, 17, 1)), 128, 8, 2)


@functools.lru_cache(maxsize=None)
def _tables(d, dtype):
    """cos / sin [ROWS, d / 2] of the dtype on the CPU from a seeded inv_freq around theta = 10000: made once, never written."""
    g = torch.Generator().manual_seed(d)
    inv_freq = 10000.0 ** (-torch.arange(0, d, 2, dtype=torch.float64) / d) * (1 + 0.01 * torch.rand(d // 2, generator=g, dtype=torch.float64))
    ang = torch.arange(ROWS, dtype=torch.float64)[:, None] * inv_freq
    return ang.cos().to(dtype), ang.sin().to(dtype)


@functools.lru_cache(maxsize=None)
def _rope(d, dtype):
    return tuple(t.to(DEV) for t in _tables(d, dtype))


def _rot(x, pos):
    """The comparator: x [tokens, heads, d] rotated to pos [tokens]."""
    dt, h = x.dtype, x.shape[-1] // 2
    cos, sin = (t[torch.as_tensor(pos, dtype=torch.long)].double()[:, None] for t in _tables(x.shape[-1], dt))
    lo, hi = x[..., :h].cpu().double(), x[..., h:].cpu().double()
    rn = lambda t: t.to(dt).double()
    return torch.cat([rn(rn(lo * cos) + rn(-hi * sin)), rn(rn(hi * cos) + rn(lo * sin))], -1).to(dt).to(DEV)


@functools.lru_cache(maxsize=None)
def _raws(name, dtype):
    if name in SETS:
        return _raw(name, dtype)
    (r1, r2), d, _, hk = GEOMS[name]
    return tuple(tuple(x.to(DEV) for x in KV._kv((1, hk, a + b, d), dtype, 3000 + i, 2.0)) for i, (a, b) in enumerate(zip(r1, r2)))


def _pools(name, dtype, n, cfg=CFG, bits=None):
    """n pools with room for the set's two rounds and one more key, the first one dirty; the sequences' ids, alike in all."""
    from lqer_amd import PagedKVCache

    (r1, r2), d, _, hk = GEOMS[name]
    need = [pages_of(a + b + 1) for a, b in zip(r1, r2)]
    pools = [PagedKVCache(sum(need), len(need), hk, d, cfg, cfg, dtype, DEV, max_pages_per_seq=max(need), code_bits=bits) for _ in range(n)]
    pools[0].buf.fill_(0xFF)
    seqs = [[p.alloc() for _ in need] for p in pools]
    assert all(s == seqs[0] for s in seqs)
    return pools, seqs[0]


def _step(name, dtype, at, counts, seed):
    """The packed raw k, v of the sequences' next counts[b] keys, queries for them, and the positions length + j."""
    _, d, h, _ = GEOMS[name]
    k, v = (_packed([r[i] for r in _raws(name, dtype)], at, counts) for i in (0, 1))
    return F._randn((sum(counts), h, d), dtype, seed, 3.0).to(DEV), k, v, [lo + j for lo, c in zip(at, counts) for j in range(c)]


def _same(got, ref, seqs, what):
    for i, s in enumerate(seqs):
        t = got.length(s)
        assert t == ref.length(s)
        if t:
            _same_live_bytes(got.to_dense(s), ref.to_dense(s), t, f"{what}: sequence {i} ({t} keys)")
            for a, b in zip(got.dequantized(s), ref.dequantized(s)):
                assert torch.equal(a, b), (what, i, t)


CASES1 = [("A", F16, CFG, None), ("A", BF16, CFG, None), ("A", F32, CFG, None), ("B", F16, CFG, None), ("A", F16, CFG4, 4), ("G", BF16, CFG, None)]


@pytest.mark.parametrize("name, dtype, cfg, bits", CASES1, ids=[f"{n}-{DT_ID[dt]}" + ("-nibble" if b else "") for n, dt, _, b in CASES1])
def test_append_rope_bits(name, dtype, cfg, bits):
    """Two ragged rounds (counts of 0, a block closed exactly, blocks left open in the first and in a later block of a call) against a
    pool fed the comparator's keys; the rotated queries; then one more key, raw, to both: the staging rows held the rotated keys."""
    rounds, d, _, hk = GEOMS[name]
    (rag, ref), seqs = _pools(name, dtype, 2, cfg, bits)
    at = [0] * len(seqs)
    for i, counts in enumerate(rounds):
        q, k, v, pos = _step(name, dtype, at, counts, 50 + i)
        q_rot = rag.append_ragged_rope(seqs, q, k, v, counts, _rope(d, dtype))
        ref.append_ragged(seqs, _rot(k, pos), v, counts)
        assert q_rot.shape == q.shape and torch.equal(u8(q_rot), u8(_rot(q, pos))), f"round {i}: rotated queries"
        at = [lo + c for lo, c in zip(at, counts)]
    _same(rag, ref, seqs, "after two rounds")
    k1, v1 = (x.to(DEV) for x in KV._kv((len(seqs), hk, 1, d), dtype, 6000, 2.0))
    rag.append(seqs, k1, v1), ref.append(seqs, k1, v1)
    _same(rag, ref, seqs, "after one more key")


def test_positions():
    """positions=None is positions = length + j; a draft tree's base + depth - repeated, not monotonic - rotates by the gathered rows."""
    name, dtype = "A", F16
    (r1, _), d, _, _ = GEOMS[name]
    (rag, exp, ref), seqs = _pools(name, dtype, 3)
    q, k, v, pos = _step(name, dtype, [0] * len(seqs), r1, 60)
    q_exp = exp.append_ragged_rope(seqs, q, k, v, r1, _rope(d, dtype), positions=torch.tensor(pos, dtype=torch.int32, device=DEV))
    assert torch.equal(u8(rag.append_ragged_rope(seqs, q, k, v, r1, _rope(d, dtype))), u8(q_exp))
    ref.append_ragged(seqs, _rot(k, pos), v, r1)
    _same(exp, ref, seqs, "explicit length + j"), _same(rag, ref, seqs, "no positions")
    depth = {0: (), 8: (0, 1, 2, 1, 2, 3, 3, 2), 5: (0, 1, 1, 2, 2), 3: (0, 1, 1)}
    counts = (0, 8, 0, 5, 3)
    q, k, v, _ = _step(name, dtype, r1, counts, 61)
    pos = [lo + dep for lo, c in zip(r1, counts) for dep in depth[c]]
    q_rot = rag.append_ragged_rope(seqs, q, k, v, counts, _rope(d, dtype), positions=torch.tensor(pos, dtype=torch.int32, device=DEV))
    ref.append_ragged(seqs, _rot(k, pos), v, counts)
    assert torch.equal(u8(q_rot), u8(_rot(q, pos)))
    _same(rag, ref, seqs, "a draft tree")


def test_in_place_and_k_only():
    """out=q and q=None against the out-of-place call - whose q, k and out start 2 bytes off a 16-byte boundary: the element-wise loads
    and stores."""
    name, dtype = "A", BF16
    (r1, _), d, _, _ = GEOMS[name]
    (a, b, c), seqs = _pools(name, dtype, 3)
    q, k, v, pos = _step(name, dtype, [0] * len(seqs), r1, 70)
    off = lambda t: torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape).copy_(t)
    q_rot = a.append_ragged_rope(seqs, off(q), off(k), v, r1, _rope(d, dtype), out=off(q))
    assert q_rot.data_ptr() % 16 == 2 and torch.equal(u8(q_rot), u8(_rot(q, pos)))
    qi = q.clone()
    assert b.append_ragged_rope(seqs, qi, k, v, r1, _rope(d, dtype), out=qi) is qi and torch.equal(u8(qi), u8(q_rot))
    assert c.append_ragged_rope(seqs, None, k, v, r1, _rope(d, dtype)) is None
    _same(b, a, seqs, "in place"), _same(c, a, seqs, "K alone")

"""The library calls of the paged pool's host layer are ASSEMBLED - the bindings from named pieces (lqer_amd/_lib.py), the argument
tuples of the seven attention entries by one builder (lqer_amd.kvcache._paged_args) - so this pins what is no longer spelled out, with
no GPU: a *_window binding is its sibling's plus one int64, and every entry's tuple has the length and the types of its binding and
the right value under each parameter name of the header's declaration."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from lqer_amd import PagedKVCache, _lib, kvcache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = _lib.SIGNATURES


def test_a_window_binding_is_its_siblings_plus_one_int64():
    for base in ("lqer_attention_q_paged", "lqer_attention_q_decode_paged", "lqer_attention_q_paged_ragged"):
        assert SIG[base + "_window"][0] is SIG[base][0] is C.c_int
        assert SIG[base + "_window"][1] == SIG[base][1] + [C.c_int64]
    assert SIG["lqer_attention_q_decode_paged_ragged"] == SIG["lqer_attention_q_paged_ragged_window"]


def _host_cache(window, **kw):
    """test_kv_ragged_cpu's host cache - buffers in host memory, launches that do nothing - holding sequences of 20 and 5 keys: the
    table's room is 256 keys and the longest length rounds up to 128, so the two max_len rules differ."""
    with open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")) as fh:
        cfg = json.load(fh)
    cache = PagedKVCache(8, 4, 2, 16, cfg, cfg, torch.float16, "cpu", max_pages_per_seq=16, window=window, **kw)
    cache._launch_append = cache._launch_append_ragged = lambda *a: None
    seqs = [cache.alloc(), cache.alloc()]
    for s, n in zip(seqs, (20, 5)):
        cache.append([s], torch.zeros(1, 2, n, 16, dtype=torch.float16), torch.zeros(1, 2, n, 16, dtype=torch.float16))
    return cache, seqs


def _names(entry):
    """The parameter names of the entry's declaration in the header, in order."""
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % entry, fh.read()).group(1)
    return [re.findall(r"[A-Za-z_]\w*", piece)[-1] for piece in decl.split(",")]


UNIFORM, RAGGED = dict(S=3), dict(counts=[3, 1])


@pytest.mark.parametrize("entry, base, window, shape, max_len", [
    ("lqer_attention_q_decode_paged", kvcache.PAGED_DECODE, None, UNIFORM, 256),
    ("lqer_attention_q_decode_paged_window", kvcache.PAGED_DECODE, 16, UNIFORM, 256),
    ("lqer_attention_q_paged", kvcache.PAGED_PREFILL, None, UNIFORM, 128),
    ("lqer_attention_q_paged_window", kvcache.PAGED_PREFILL, 16, UNIFORM, 128),
    ("lqer_attention_q_paged_ragged", kvcache.RAGGED_PREFILL, None, RAGGED, 128),
    ("lqer_attention_q_paged_ragged_window", kvcache.RAGGED_PREFILL, 16, RAGGED, 128),
    ("lqer_attention_q_decode_paged_ragged", kvcache.RAGGED_DECODE, None, RAGGED, 128),
    ("lqer_attention_q_decode_paged_ragged", kvcache.RAGGED_DECODE, 16, RAGGED, 128),
])
def test_the_argument_tuple_of_every_entry(entry, base, window, shape, max_len):
    cache, seqs = _host_cache(window, **({"max_query_rows": 8} if window else {}))
    slots = cache.pt.slots(seqs)
    lens = [cache.pt.lengths[x] for x in slots]
    assert lens == [20, 5] and cache.pt.max_len == 256
    q = torch.zeros((4, 4, 16) if "counts" in shape else (2, 4, 3, 16), dtype=torch.float16)
    out = torch.empty_like(q)
    name, args = kvcache._paged_args(base, q, out, None, cache, slots, lens, 0.25, True, window, 0, 0, None, **shape)
    assert name == entry
    argtypes = SIG[entry][1]
    assert len(args) == len(argtypes)
    for t, a in zip(argtypes, args):
        t.from_param(a)  # (raises for a value the binding would not take)
    names = _names(entry)
    assert len(names) == len(args)
    got = dict(zip(names, args))
    want = dict(pages=8, slots=4, table_stride=16, batch=2, heads=4, kv_heads=2, D=16, causal=1, max_len=max_len, q=q.data_ptr(),
                out=out.data_ptr(), row_stats=None, pool=cache.buf.data_ptr(), pool_bytes=cache.buf.numel(), dtype=_lib.F16, scaling=0.25,
                block_table=cache.table.data_ptr(), seq_slots=cache._slots.data_ptr(), lens=cache._lens.data_ptr(), workspace=0,
                workspace_bytes=0, stream=None)
    if "counts" in shape:
        want.update(max_s=3, total=4, q_starts=cache._starts.data_ptr())
        assert "S" not in got and cache._starts[:3].tolist() == [0, 3, 4]
        assert list(got["q_strides"]) == [64, 16] and list(got["out_strides"]) == [64, 16]
    else:
        want.update(S=3)
        assert list(got["q_strides"]) == [192, 48, 16] and list(got["out_strides"]) == [192, 48, 16]
    if entry.endswith("_window") or base == kvcache.RAGGED_DECODE:
        want.update(window=window or 0)
    else:
        assert "window" not in got
    assert {k: got[k] for k in want} == want
    assert cache._slots[:2].tolist() == slots and cache._lens[:2].tolist() == lens  # the call's metadata, where the pointers point

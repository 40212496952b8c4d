"""Rotary position embedding inside the paged pool's append (lqer_kv_pool_append_rope: csrc/kv_rope.hip; lqer_amd.kvcache.rope_tables,
PagedKVCache.append_ragged_rope), the part that needs no GPU: the export is declared with the argument list it is bound with, every
refusal comes with its code and a message before anything touches the device, and rope_tables keeps the first half of the model's own
cos / sin."""
import ctypes as C
import os
import re

import pytest
import torch

from lqer_amd import _lib
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, POOL_OK, _fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lqer_kv_pool_append_rope"
pair = lambda a, b: (C.c_int64 * 2)(a, b)


def test_export_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    decl = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, hdr)
    assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 32
    getattr(_lib.lib(), NAME)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # an additive export
    # lqer_kv_pool_append_ragged's list with (q, q_out, two stride pairs, heads) in front of k_new and (cos, sin, rope_rows, positions) behind v_strides
    rg, rp = _lib.SIGNATURES["lqer_kv_pool_append_ragged"][1], _lib.SIGNATURES[NAME][1]
    vp, i64, sp = C.c_void_p, C.c_int64, C.POINTER(C.c_int64)
    assert rp == rg[:11] + [vp, vp, sp, sp, i64] + rg[11:15] + [vp, vp, i64, vp] + rg[15:]


def _call(pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000, lens=0x400000, max_len=40, starts=0x500000,
          max_n=3, q=0x60000, q_out=0x70000, qs=True, os_=True, heads=8, k=0x20000, v=0x30000, ks=True, vs=True, cos=0x80000, sin=0x90000, rows=64,
          positions=None, dtype=_lib.F16, batch=2, kv=4, D=64, total=4, k_fmt=None, v_fmt=None):
    L = _lib.lib()
    k_fmt, v_fmt = k_fmt or _fmt(), v_fmt or _fmt()
    st, qst = pair(kv * D, D), pair(heads * D, D)
    rc = getattr(L, NAME)(pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, starts, max_n, q, q_out, qst if qs else None,
                          qst if os_ else None, heads, k, v, st if ks else None, st if vs else None, cos, sin, rows, positions, dtype, batch, kv, D,
                          total, C.byref(k_fmt) if k_fmt != "null" else None, C.byref(v_fmt) if v_fmt != "null" else None, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    # the additions
    ("null cos", dict(cos=None), E_INVALID),
    ("null sin", dict(sin=None), E_INVALID),
    ("rope_rows = 0", dict(rows=0), E_INVALID),
    ("cos not 16-byte aligned", dict(cos=0x80008), E_INVALID),
    ("sin not 16-byte aligned", dict(sin=0x90002), E_INVALID),
    ("max_len + max_n > rope_rows without positions", dict(rows=42), E_INVALID),
    ("q null with heads", dict(q=None), E_INVALID),
    ("q without heads", dict(heads=0), E_INVALID),
    ("q without q_out", dict(q_out=None), E_INVALID),
    ("null q strides", dict(qs=False), E_INVALID),
    ("null q_out strides", dict(os_=False), E_INVALID),
    ("total x heads beyond one launch grid", dict(total=1 << 28, heads=16), E_UNSUPPORTED),
    # lqer_kv_pool_append_ragged's, through the check the two entries share
    ("null new_starts", dict(starts=None), E_INVALID),
    ("max_n > max_len", dict(max_n=41, rows=128), E_INVALID),
    ("null k strides", dict(ks=False), E_INVALID),
    ("null lens", dict(lens=None), E_INVALID),
    ("short pool", dict(pool_bytes=POOL_OK - 1), E_INVALID),
    ("null k_new", dict(k=None), E_INVALID),
    ("unknown dtype", dict(dtype=9), E_INVALID),
    ("block 32", dict(k_fmt=_fmt(32)), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("beyond one launch grid", dict(batch=1 << 20, max_n=1 << 20, max_len=1 << 20, stride=1 << 16, rows=1 << 22), E_UNSUPPORTED),
])
def test_refusals_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _call(**kwargs)
    assert rc == want, (case, rc, msg)
    assert ("KV pool" in msg or "KV cache" in msg or "quantizer" in msg) and len(msg) > 20, (case, msg)
    if "quantizer" not in msg:
        assert msg.startswith("kv_pool_append_rope:"), (case, msg)  # the message names the call


def test_nothing_to_do_is_ok_and_positions_lift_the_row_bound():
    assert _call(batch=0)[0] == 0 and _call(total=0)[0] == 0 and _call(total=0, q=None, q_out=None, heads=0)[0] == 0
    assert _call(total=0, rows=1, positions=0xa0000)[0] == 0 and _call(total=0, rows=43)[0] == 0


def test_rope_tables_are_the_first_half_of_the_models():
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding

    from lqer_amd import rope_tables

    cfg = LlamaConfig(hidden_size=64, num_attention_heads=2, num_hidden_layers=1, intermediate_size=64, vocab_size=32, max_position_embeddings=64)
    rot = LlamaRotaryEmbedding(cfg)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        cos, sin = rope_tables(rot, 40, dtype, "cpu")
        want_cos, want_sin = rot(torch.empty(0, dtype=dtype), torch.arange(40)[None])
        assert want_cos.shape == (1, 40, 32) and torch.equal(want_cos[..., :16], want_cos[..., 16:])  # HF duplicates the halves
        for got, want in ((cos, want_cos), (sin, want_sin)):
            assert got.shape == (40, 16) and got.dtype == dtype and got.is_contiguous() and torch.equal(got, want[0, :, :16])

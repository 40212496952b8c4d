"""Fused quantized attention (csrc/attn_q.hip), the part that needs no GPU: the two C-ABI exports are bound and declared, the
workspace size follows the header's layout formula, bad arguments are refused with a message before anything touches the
device, CPU tensors raise, and the default attention implementation is unchanged."""
import ctypes as C
import os
import re

import pytest
import torch

from lqer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2


def _header() -> str:
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        return fh.read()


def test_exports_bound_and_declared():
    hdr = _header()
    for name in ("lqer_attention_q_workspace_bytes", "lqer_attention_q"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert "llama_decoder.py:259-297" in hdr and "opt_decoder.py:125,190" in hdr
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION
    assert re.search(r"#define\s+LQER_ABI_VERSION\s+14\b", hdr)


def _ws(batch, heads, kv, S, T, D):
    return _lib.lib().lqer_attention_q_workspace_bytes(batch, heads, kv, S, T, D)


def _formula(batch, kv, T, D):
    """include/lqer_hip.h: [K image: batch kv x (T up to 128) x (D up to 64) bf16][V image: batch kv x 128 x (T up to 64) bf16],
    each part rounded up to 256 bytes."""
    up = lambda v, m: (v + m - 1) // m * m
    return up(batch * kv * up(T, 128) * up(D, 64) * 2, 256) + up(batch * kv * 128 * up(T, 64) * 2, 256)


def test_workspace_bytes():
    for batch, heads, kv, S, T, D in [(1, 32, 32, 2048, 2048, 128), (4, 8, 2, 200, 328, 64), (2, 4, 4, 1, 37, 16), (3, 6, 3, 77, 1, 48)]:
        assert _ws(batch, heads, kv, S, T, D) == _formula(batch, kv, T, D)
    base = _ws(2, 8, 2, 100, 300, 64)
    assert _ws(3, 8, 2, 100, 300, 64) > base and _ws(2, 8, 2, 100, 600, 64) > base  # monotone in batch and T
    assert _ws(2, 16, 2, 100, 300, 64) == base == _ws(2, 2, 2, 100, 300, 64)  # the images belong to the kv heads
    assert _ws(2, 8, 2, 4000, 300, 64) == base  # nothing of [S, T] size, nothing per query
    assert _ws(2, 8, 4, 100, 300, 64) > base
    assert _ws(0, 8, 2, 100, 300, 64) == 0 and _ws(2, 8, 2, 100, 0, 64) == 0


def _fmt(block=16, width=8, kind=_lib.Q_MXINT):
    return _lib.QFmt(kind, width, block, 8, 127)


def _call(q=0x10000, k=0x20000, v=0x30000, out=0x40000, ws=0x50000, ws_bytes=None, batch=1, heads=4, kv=4, S=8, T=8, D=64, fmts=None, mask=None,
          causal=0):
    L = _lib.lib()
    tri = lambda a, b, c: (C.c_int64 * 3)(a, b, c)
    fmts = fmts or [_fmt()] * 4
    if ws_bytes is None:
        ws_bytes = _ws(batch, heads, kv, S, T, D)
    rc = L.lqer_attention_q(q, k, v, mask, out, None, _lib.F16, batch, heads, kv, S, T, D, tri(heads * S * D, S * D, D), tri(kv * T * D, T * D, D),
                            tri(kv * T * D, T * D, D), tri(0, 0, T) if mask else None, tri(heads * S * D, S * D, D), 0.125, causal,
                            C.byref(fmts[0]), C.byref(fmts[1]), C.byref(fmts[2]), C.byref(fmts[3]), ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("null q", dict(q=None), E_INVALID),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("short workspace", dict(ws_bytes=_formula(1, 4, 8, 64) - 1), E_INVALID),
    ("mask and causal", dict(mask=0x60000, causal=1), E_INVALID),
])
def test_argument_validation_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _call(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)


def test_cpu_tensors_raise_like_matmul_flexible():
    import json

    from lqer_amd import attention_flexible, matmul_flexible

    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    q, k, v = torch.randn(1, 2, 5, 16), torch.randn(1, 2, 7, 16), torch.randn(1, 2, 7, 16)
    with pytest.raises(RuntimeError) as e_mm:
        matmul_flexible(q[0], k[0].transpose(1, 2), cfg)
    with pytest.raises(RuntimeError) as e_at:
        attention_flexible(q, k, v, cfg, cfg, 0.25)
    assert str(e_at.value) == str(e_mm.value)
    assert attention_flexible.route(q, k, v, cfg, cfg) == "unfused"


def test_default_implementation_unchanged():
    import json

    from transformers import LlamaConfig, LlamaForCausalLM

    from lqer_amd import attention as A

    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    torch.manual_seed(0)
    mk = lambda: LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                                              num_key_value_heads=2, vocab_size=64, max_position_embeddings=32)).eval()
    assert A.IMPLEMENTATION == "lqer_eager"
    model = A.enable_quantized_attention(mk(), {"matmul": cfg})
    assert model.config._attn_implementation == "lqer_eager"
    fused = A.enable_quantized_attention(mk(), {"matmul": cfg}, fused=True)
    assert fused.config._attn_implementation == "lqer_fused" == A.IMPLEMENTATION_FUSED
    assert fused.model.layers[0].self_attn._lqer_matmul_cfg[0]["x_quantizer"]["block_size"] == [1, 16]

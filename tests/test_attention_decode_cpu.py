"""The decode kernel of the fused quantized attention (csrc/attn_decode.hip), the part that needs no GPU: the two C-ABI exports are
bound and declared, the workspace size follows the header's layout formula, bad arguments are refused with a message before anything
touches the device, and the Python side names the kernel it would run."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from lqer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
CFG = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))


def test_exports_bound_and_declared():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in ("lqer_attention_q_decode_workspace_bytes", "lqer_attention_q_decode"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(_lib.lib(), name)
    assert _lib.SIGNATURES["lqer_attention_q_decode"] == _lib.SIGNATURES["lqer_attention_q"]  # the same argument list
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports


def _ws(batch, heads, kv, S, T, D):
    return _lib.lib().lqer_attention_q_decode_workspace_bytes(batch, heads, kv, S, T, D)


def _formula(batch, heads, S, T, D):
    """include/lqer_hip.h: rows = batch heads S, C = 16 min(max(ceil(T / 256), 1), 8), nch = ceil(T / C):
    [S2 fp32: rows x nch C][chunk statistics fp32: rows x nch x 2][partial outputs fp32: rows x nch x D], each rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256
    C_ = 16 * min(max(-(-T // 256), 1), 8)
    nch, rows = -(-T // C_), batch * heads * S
    return up(rows * nch * C_ * 4) + up(rows * nch * 2 * 4) + up(rows * nch * D * 4)


def test_workspace_bytes():
    for batch, heads, kv, S, T, D in [(1, 32, 32, 1, 2048, 128), (8, 32, 8, 1, 4096, 128), (2, 4, 2, 5, 37, 80), (3, 6, 3, 8, 300, 48)]:
        assert _ws(batch, heads, kv, S, T, D) == _formula(batch, heads, S, T, D)
    assert _ws(1, 32, 32, 1, 2048, 128) == _ws(1, 32, 8, 1, 2048, 128)  # sized by the query rows, not by the kv heads
    assert _ws(0, 8, 2, 1, 300, 64) == 0 and _ws(2, 8, 2, 1, 0, 64) == 0


def _fmt(block=16, width=8, kind=_lib.Q_MXINT):
    return _lib.QFmt(kind, width, block, 8, 127)


def _call(q=0x10000, k=0x20000, v=0x30000, out=0x40000, ws=0x50000, ws_bytes=None, batch=1, heads=4, kv=4, S=1, T=40, D=64, fmts=None, mask=None,
          causal=0):
    L = _lib.lib()
    tri = lambda a, b, c: (C.c_int64 * 3)(a, b, c)
    fmts = fmts or [_fmt()] * 4
    if ws_bytes is None:
        ws_bytes = max(_ws(batch, heads, kv, S, T, D), 1 << 20)
    rc = L.lqer_attention_q_decode(q, k, v, mask, out, None, _lib.F16, batch, heads, kv, S, T, D, tri(heads * S * D, S * D, D),
                                   tri(kv * T * D, T * D, D), tri(kv * T * D, T * D, D), tri(0, 0, T) if mask else None, tri(heads * S * D, S * D, D),
                                   0.125, causal, C.byref(fmts[0]), C.byref(fmts[1]), C.byref(fmts[2]), C.byref(fmts[3]), ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want", [
    ("S = 9", dict(S=9), E_UNSUPPORTED),
    ("block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), E_UNSUPPORTED),
    ("width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("minifloat", dict(fmts=[_fmt(), _lib.QFmt(_lib.Q_MINIFLOAT, 8, 16, 4, 7), _fmt(), _fmt()]), E_UNSUPPORTED),
    ("D = 24", dict(D=24), E_UNSUPPORTED),
    ("D = 144", dict(D=144), E_UNSUPPORTED),
    ("null q", dict(q=None), E_INVALID),
    ("null k", dict(k=None), E_INVALID),
    ("null v", dict(v=None), E_INVALID),
    ("null out", dict(out=None), E_INVALID),
    ("null workspace", dict(ws=None), E_INVALID),
    ("workspace not 16-byte aligned", dict(ws=0x50008), E_INVALID),
    ("heads % kv_heads", dict(heads=6, kv=4), E_INVALID),
    ("short workspace", dict(ws_bytes=_formula(1, 4, 1, 40, 64) - 1), E_INVALID),
    ("mask and causal", dict(mask=0x60000, causal=1), E_INVALID),
])
def test_argument_validation_before_any_gpu_call(case, kwargs, want):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text.
    (No GPU is needed, and none is touched.)"""
    rc, msg = _call(**kwargs)
    assert rc == want, (case, rc, msg)
    assert "attention" in msg and len(msg) > 20, (case, msg)


def test_kernel_tag_and_argument_on_cpu_tensors():
    from lqer_amd import attention_flexible

    q, k, v = torch.randn(1, 2, 1, 16), torch.randn(1, 2, 7, 16), torch.randn(1, 2, 7, 16)
    assert attention_flexible.kernel(q, k, v, CFG, CFG) is None  # CPU tensors: the unfused route (which then raises, as matmul_flexible)
    assert attention_flexible.route(q, k, v, CFG, CFG) == "unfused"
    with pytest.raises(ValueError):
        attention_flexible(q, k, v, CFG, CFG, 0.25, kernel="bogus")

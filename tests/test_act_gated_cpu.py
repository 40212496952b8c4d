"""The gated-MLP entries of the C ABI (lqer_quantize_act_xa_gated, lqer_linear_forward_gated: csrc/act_gated.hip), the part that needs no
GPU: both exports are declared, exported and bound, additive to ABI 14, and every refusal comes with its code and a text of its own
before anything touches the device."""
import ctypes as C
import os
import re

import pytest

from bench import MXINT_Q
from lqer_amd import LinearFlexibleLqer, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
NAMES = ("lqer_quantize_act_xa_gated", "lqer_linear_forward_gated")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\s*\(" % name, hdr)
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # additive exports
    assert "#define LQER_ACT_SILU 0" in hdr and "#define LQER_ACT_RELU 1" in hdr and (_lib.ACT_SILU, _lib.ACT_RELU) == (0, 1)
    # the forward takes lqer_linear_forward's operands behind (desc, gate, up, act, dtype, M, ld_gate, ld_up)
    assert _lib.SIGNATURES[NAMES[1]][1][8:] == _lib.SIGNATURES["lqer_linear_forward"][1][5:]


def _call(entry, K=512, r=32, gate=0x100000, up=0x200000, act=0, dtype=_lib.F16, M=8, ldg=None, ldu=None, a_t=0x300000, a_limbs=-2, xq=0x400000,
          xaq=0x500000, fmt=None, ws_bytes=1 << 30):
    mod = LinearFlexibleLqer(K, 256, bias=False, q_config=MXINT_Q, l_config={"rank": r})
    desc = mod._desc()
    for field, val in (fmt or {}).items():
        setattr(getattr(desc, field[0]), field[1], val)
    L = _lib.lib()
    lead = (C.byref(desc), gate, up, act, dtype, M, K if ldg is None else ldg, K if ldu is None else ldu)
    rc = (L.lqer_quantize_act_xa_gated(*lead, a_t, a_limbs, xq, xaq, None) if entry == "act" else
          L.lqer_linear_forward_gated(*lead, 0x600000, a_t, 0x700000, a_limbs, 1, None, 0x800000, 256, xq, ws_bytes, None))
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("entry", ["act", "forward"])
@pytest.mark.parametrize("case, kwargs, want, text", [
    ("null gate", dict(gate=None), E_INVALID, "null gate"),
    ("negative M", dict(M=-1), E_INVALID, "negative token count"),
    ("ld_gate < K", dict(ldg=504), E_INVALID, "row stride 504 of gate"),
    ("ld_up < K", dict(ldu=256), E_INVALID, "row stride 256 of up"),
    ("unknown act", dict(act=2), E_INVALID, "unknown activation 2"),
    ("a_limbs = 1", dict(a_limbs=1), E_INVALID, "a_limbs 1"),
    ("rank without A^T", dict(a_t=None), E_INVALID, "no A^T image"),
    ("fp32 input", dict(dtype=_lib.F32), E_UNSUPPORTED, "fp32 gate / up"),
    ("x in blocks of 32", dict(fmt={("x_fmt", "block"): 32}), E_UNSUPPORTED, "blocks of 16"),
    ("x pass-through", dict(fmt={("x_fmt", "kind"): _lib.Q_PASSTHROUGH}), E_UNSUPPORTED, "blocks of 16"),
    ("8-bit weight", dict(fmt={("w_fmt", "width"): 8}), E_UNSUPPORTED, "weights of 5..8 bits"),
    ("K = 520", dict(K=520), E_UNSUPPORTED, "multiple of 16"),
    ("gate not 16-byte aligned", dict(gate=0x100008), E_UNSUPPORTED, "16-byte aligned"),
    ("ld_up not 16-byte aligned", dict(ldu=516), E_UNSUPPORTED, "16-byte aligned"),
    ("padded rank 48", dict(r=48), E_UNSUPPORTED, "padded rank must be 16, 32 or 64"),
    ("A_out in blocks of 12", dict(fmt={("a_out_fmt", "block"): 12}), E_UNSUPPORTED, "A_out blocks"),
])
def test_refusals_before_any_gpu_call(entry, case, kwargs, want, text):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text."""
    rc, msg = _call(entry, **kwargs)
    assert rc == want and text in msg, (case, rc, msg)
    assert ("linear_forward_gated" if entry == "forward" and want == E_INVALID else "_gated") in msg, (case, msg)


def test_entry_specific_refusals():
    assert _call("act", xq=None) == (E_INVALID, "quantize_act_xa_gated: null activation image")
    assert _call("act", xaq=None) == (E_INVALID, "quantize_act_xa_gated: null xaq")
    rc, msg = _call("forward", ws_bytes=4096)
    assert rc == E_WORKSPACE and "linear_forward_gated: workspace 4096 B" in msg

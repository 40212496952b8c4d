"""The fused-RMSNorm entries of the C ABI (lqer_quantize_act_xa_normed, lqer_linear_forward_normed: csrc/act_normed.hip), the part that
needs no GPU: both exports are declared, exported and bound, additive to ABI 14, every refusal of the header's list comes with its
code and a text of its own before anything touches the device, and quantize_model(fuse_norm=True) refuses a LayerNorm model."""
import ctypes as C
import os
import re

import pytest

from bench import MXINT_Q, OPT_Q
from lqer_amd import LinearFlexibleLqer, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
NAMES = ("lqer_quantize_act_xa_normed", "lqer_linear_forward_normed")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\s*\(" % name, hdr)
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # additive exports
    # the forward takes lqer_linear_forward's operands behind (desc, h, norm_weight, eps, dtype, M, ld_h)
    assert _lib.SIGNATURES[NAMES[1]][1][7:] == _lib.SIGNATURES["lqer_linear_forward"][1][5:]


def _call(entry, K=512, r=32, h=0x100000, nw=0x200000, eps=1e-5, dtype=_lib.F16, M=8, ldh=None, a_t=0x300000, a_limbs=-2, xq=0x400000,
          xaq=0x500000, fmt=None, ws_bytes=1 << 30):
    mod = LinearFlexibleLqer(K, 256, bias=False, q_config=MXINT_Q, l_config={"rank": r})
    desc = mod._desc()
    for field, val in (fmt or {}).items():
        setattr(getattr(desc, field[0]), field[1], val)
    L = _lib.lib()
    lead = (C.byref(desc), h, nw, eps, dtype, M, K if ldh is None else ldh)
    rc = (L.lqer_quantize_act_xa_normed(*lead, a_t, a_limbs, xq, xaq, None) if entry == "act" else
          L.lqer_linear_forward_normed(*lead, 0x600000, a_t, 0x700000, a_limbs, 1, None, 0x800000, 256, xq, ws_bytes, None))
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("entry", ["act", "forward"])
@pytest.mark.parametrize("case, kwargs, want, text", [
    ("null h", dict(h=None), E_INVALID, "null hidden state"),
    ("null norm weight", dict(nw=None), E_INVALID, "null norm weight"),
    ("negative M", dict(M=-1), E_INVALID, "negative token count"),
    ("ld_h < K", dict(ldh=504), E_INVALID, "row stride 504 of h"),
    ("eps < 0", dict(eps=-1e-5), E_INVALID, "finite and >= 0"),
    ("eps = inf", dict(eps=float("inf")), E_INVALID, "finite and >= 0"),
    ("eps = nan", dict(eps=float("nan")), E_INVALID, "finite and >= 0"),
    ("a_limbs = 1", dict(a_limbs=1), E_INVALID, "a_limbs 1"),
    ("rank without A^T", dict(a_t=None), E_INVALID, "no A^T image"),
    ("fp32 input", dict(dtype=_lib.F32), E_UNSUPPORTED, "fp32 h"),
    ("x in blocks of 32", dict(fmt={("x_fmt", "block"): 32}), E_UNSUPPORTED, "blocks of 16"),
    ("x pass-through", dict(fmt={("x_fmt", "kind"): _lib.Q_PASSTHROUGH}), E_UNSUPPORTED, "blocks of 16"),
    ("8-bit weight", dict(fmt={("w_fmt", "width"): 8}), E_UNSUPPORTED, "weights of 5..8 bits"),
    ("K = 520", dict(K=520), E_UNSUPPORTED, "multiple of 16"),
    ("K = 8208", dict(K=8208), E_UNSUPPORTED, "above 8192"),
    ("h not 16-byte aligned", dict(h=0x100008), E_UNSUPPORTED, "16-byte aligned"),
    ("norm weight not 16-byte aligned", dict(nw=0x200004), E_UNSUPPORTED, "16-byte aligned"),
    ("ld_h not 16-byte aligned", dict(ldh=516), E_UNSUPPORTED, "16-byte aligned"),
    ("padded rank 80", dict(r=80), E_UNSUPPORTED, "padded rank must be 16, 32, 48, 64, 96 or 128"),
    ("A_out in blocks of 12", dict(fmt={("a_out_fmt", "block"): 12}), E_UNSUPPORTED, "A_out blocks"),
])
def test_refusals_before_any_gpu_call(entry, case, kwargs, want, text):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text."""
    rc, msg = _call(entry, **kwargs)
    assert rc == want and text in msg, (case, rc, msg)
    assert ("linear_forward_normed" if entry == "forward" and want == E_INVALID else "_normed") in msg, (case, msg)


def test_entry_specific_refusals():
    assert _call("act", xq=None) == (E_INVALID, "quantize_act_xa_normed: null activation image")
    assert _call("act", xaq=None) == (E_INVALID, "quantize_act_xa_normed: null xaq")
    rc, msg = _call("forward", ws_bytes=4096)
    assert rc == E_WORKSPACE and "linear_forward_normed: workspace 4096 B" in msg


def test_fuse_norm_refuses_a_layernorm_model():
    from lqer_amd.models import quantize_model
    from test_model_swap import _tiny_opt

    with pytest.raises(NotImplementedError, match="fuse_norm"):
        quantize_model(_tiny_opt(), {"linear": OPT_Q}, {"linear": {"rank": 16}}, fuse_norm=True)

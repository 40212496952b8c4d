"""lqer_linear_decode_gated without a GPU: the export is declared, exported and bound, additive to ABI 14, and every refusal of the header's
list comes with its code and its "linear_decode_gated:" text before anything touches the device."""
import ctypes as C
import os
import re

import pytest

from bench import MXINT_Q
from lqer_amd import LinearFlexibleLqer, _lib

E_INVALID, E_UNSUPPORTED = -1, -2
NAME = "lqer_linear_decode_gated"


def test_export_declared_exported_bound():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    assert NAME in _lib.SIGNATURES and re.search(r"\bint %s\s*\(" % NAME, hdr) and getattr(_lib.lib(), NAME)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # an additive export
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["lqer_linear_forward_gated"]  # the operands of the two-launch gated forward


def _call(K=512, r=32, gate=0x100000, up=0x200000, act=_lib.ACT_SILU, dtype=_lib.F16, M=8, ldg=None, ldu=None, a_limbs=1, fmt=None):
    """The pointers are made up: a call that got past validation would fault."""
    desc = LinearFlexibleLqer(K, 256, bias=False, q_config=MXINT_Q, l_config={"rank": r})._desc()
    for field, val in (fmt or {}).items():
        setattr(getattr(desc, field[0]), field[1], val)
    L = _lib.lib()
    rc = L.lqer_linear_decode_gated(C.byref(desc), gate, up, act, dtype, M, K if ldg is None else ldg, K if ldu is None else ldu, 0x600000,
                                    0x300000, 0x700000, a_limbs, 1, None, 0x800000, 256, 0x400000, 1 << 30, None)
    return rc, L.lqer_last_error().decode()


REFUSALS = [
    ("null gate", dict(gate=None), E_INVALID, "null gate"),
    ("unknown act", dict(act=2), E_INVALID, "unknown activation 2"),
    ("ld_gate < K", dict(ldg=504), E_INVALID, "row stride 504 of gate"),
    ("ld_up < K", dict(ldu=496), E_INVALID, "row stride 496 of up"),
    ("fp32 tensors", dict(dtype=_lib.F32), E_UNSUPPORTED, "fp32 gate / up"),
    ("M = 9", dict(M=9), E_UNSUPPORTED, "up to 8 tokens"),
    ("K = 520", dict(K=520), E_UNSUPPORTED, "multiple of 16"),
    ("gate not 16-byte aligned", dict(gate=0x100008), E_UNSUPPORTED, "16-byte aligned"),
    ("up not 16-byte aligned", dict(up=0x200004), E_UNSUPPORTED, "16-byte aligned"),
    ("ld_gate not 16-byte aligned", dict(ldg=516), E_UNSUPPORTED, "16-byte aligned"),
    ("ld_up not 16-byte aligned", dict(ldu=516), E_UNSUPPORTED, "16-byte aligned"),
    # what the decode route refuses: the prepared image of the large-M kernel, formats outside the route, an image past the LDS
    ("a_limbs = -2", dict(a_limbs=-2), E_UNSUPPORTED, "one-launch decode route"),
    ("x in blocks of 32", dict(fmt={("x_fmt", "block"): 32}), E_UNSUPPORTED, "one-launch decode route"),
    ("M = 7 at K = 11008", dict(K=11008, M=7), E_UNSUPPORTED, "K too long for the LDS image"),
    ("M = 5 at K = 16384", dict(K=16384, M=5, up=None, act=_lib.ACT_RELU), E_UNSUPPORTED, "K too long for the LDS image"),
]


@pytest.mark.parametrize("case, kwargs, want, text", REFUSALS)
def test_refusals_before_any_gpu_call(case, kwargs, want, text):
    rc, msg = _call(**kwargs)
    assert rc == want and text in msg and msg.startswith("linear_decode_gated:"), (case, rc, msg)

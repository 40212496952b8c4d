"""The one-launch decode entries behind a norm (lqer_linear_forward_group_normed / _layernormed, lqer_linear_decode_normed /
_layernormed: csrc/decode1.hip's NORM instantiations), the part that needs no GPU: the four exports are declared, exported and bound,
additive to ABI 14, and every refusal of the header's list comes with its code before anything touches the device."""
import ctypes as C
import os
import re

import pytest

from bench import MXINT_Q
from lqer_amd import LinearFlexibleLqer, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
NAMES = ("lqer_linear_forward_group_normed", "lqer_linear_forward_group_layernormed", "lqer_linear_decode_normed",
         "lqer_linear_decode_layernormed")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\s*\(" % name, hdr)
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION and "#define LQER_ABI_VERSION 14" in hdr  # additive exports
    S = _lib.SIGNATURES  # the single-Linear entries take the operands of the two-launch normed forwards
    assert S[NAMES[2]] == S["lqer_linear_forward_normed"] and S[NAMES[3]] == S["lqer_linear_forward_layernormed"]


def _call(entry, K=512, r=32, h=0x100000, nw=0x200000, nb=0x280000, eps=1e-5, dtype=_lib.F16, M=8, ldh=None, a_limbs=1, fmt=None):
    """entry: (group or one Linear, RMSNorm or LayerNorm).  The pointers are made up: a call that got past validation would fault."""
    group, layer = entry
    mods = [LinearFlexibleLqer(K, 256, bias=False, q_config=MXINT_Q, l_config={"rank": r}) for _ in range(2 if group else 1)]
    descs = [m._desc() for m in mods]
    for d in descs:
        for field, val in (fmt or {}).items():
            setattr(getattr(d, field[0]), field[1], val)
    L = _lib.lib()
    norm = (h, nw, nb, eps) if layer else (h, nw, eps)
    ldh = K if ldh is None else ldh
    if group:
        tab = (_lib.GroupMember * 2)()
        for i, d in enumerate(descs):
            tab[i].desc, tab[i].w_packed, tab[i].b_t, tab[i].b_limbs = C.pointer(d), 0x600000, 0x700000, 1
            tab[i].bias_q, tab[i].y, tab[i].ldy = None, 0x800000 + 0x10000 * i, 256
        fn = L.lqer_linear_forward_group_layernormed if layer else L.lqer_linear_forward_group_normed
        rc = fn(tab, 2, *norm, dtype, M, ldh, 0x300000, a_limbs, 0x400000, 1 << 30, None)
    else:
        fn = L.lqer_linear_decode_layernormed if layer else L.lqer_linear_decode_normed
        rc = fn(C.byref(descs[0]), *norm, dtype, M, ldh, 0x600000, 0x300000, 0x700000, a_limbs, 1, None, 0x800000, 256, 0x400000, 1 << 30, None)
    return rc, L.lqer_last_error().decode()


ENTRIES = {"group-rms": (True, False), "group-layer": (True, True), "one-rms": (False, False), "one-layer": (False, True)}
REFUSALS = [
    ("null h", dict(h=None), E_INVALID, ""),
    ("null norm weight", dict(nw=None), E_INVALID, "null norm weight"),
    ("ld_h < K", dict(ldh=504), E_INVALID, "row stride 504 of h"),
    ("eps < 0", dict(eps=-1e-5), E_INVALID, "finite and >= 0"),
    ("eps = nan", dict(eps=float("nan")), E_INVALID, "finite and >= 0"),
    ("fp32 input", dict(dtype=_lib.F32), E_UNSUPPORTED, "fp32 h"),
    ("M = 9", dict(M=9), E_UNSUPPORTED, "up to 8 tokens"),
    ("K = 520", dict(K=520), E_UNSUPPORTED, "multiple of 16"),
    ("K = 8208", dict(K=8208), E_UNSUPPORTED, "at most 8192"),
    ("h not 16-byte aligned", dict(h=0x100008), E_UNSUPPORTED, "16-byte aligned"),
    ("norm weight not 16-byte aligned", dict(nw=0x200004), E_UNSUPPORTED, "16-byte aligned"),
    ("ld_h not 16-byte aligned", dict(ldh=516), E_UNSUPPORTED, "16-byte aligned"),
    # what lqer_linear_forward_group / the decode route refuse: the prepared image of the large-M kernel, formats outside the route
    ("a_limbs = -2", dict(a_limbs=-2), E_UNSUPPORTED, "one-launch decode route"),
    ("x in blocks of 32", dict(fmt={("x_fmt", "block"): 32}), E_UNSUPPORTED, "one-launch decode route"),
]
LAYER_ONLY = [
    ("null norm bias", dict(nb=None), E_INVALID, "null norm bias"),
    ("norm bias not 16-byte aligned", dict(nb=0x280004), E_UNSUPPORTED, "16-byte aligned"),
]


@pytest.mark.parametrize("entry, case, kwargs, want, text",
                         [(e,) + c for e in ENTRIES for c in REFUSALS + (LAYER_ONLY if ENTRIES[e][1] else [])])
def test_refusals_before_any_gpu_call(entry, case, kwargs, want, text):
    rc, msg = _call(ENTRIES[entry], **kwargs)
    assert rc == want and text in msg and entry.split("-")[0].replace("one", "decode") in msg, (case, rc, msg)


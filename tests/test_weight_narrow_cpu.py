"""The compact image of 2- / 3-bit block_fp weights (include/lqer_hip.h "compact weight image", csrc/w_narrow.h) without a GPU: the
exports exist, the byte counts follow the formula, the host conversions round-trip byte for byte and put every bit where the header
says (read back by tests/_narrow_ref.py, an independent numpy reading of both layouts), and the host-side refusals carry a reason."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _narrow_ref as R  # noqa: E402
from lqer_amd import _lib  # noqa: E402
from lqer_amd._lib import LinearDesc, QFmt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lqer_weight_narrow_bytes", "lqer_weight_narrow", "lqer_weight_widen", "lqer_weight_narrow_host", "lqer_weight_widen_host",
       "lqer_weight_narrow_route", "lqer_linear_forward_narrow_workspace_bytes", "lqer_linear_forward_narrow", "lqer_linear_gemm_narrow")
FORMATS = [(2, 16), (2, 32), (3, 32), (3, 16), (3, 128), (2, -1), (3, 48)]  # (width, block)
SHAPES = [(48, 200), (272, 4688)]


def _wfmt(width, block, kind=_lib.Q_MXINT):
    return QFmt(kind, width, block, 8, 127)


def _aligned(nbytes):
    """A zeroed uint8 array whose data is 16-byte aligned (the C ABI's contract for images)."""
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off: off + nbytes]


def _narrow_host(img, N, K, f):
    L = _lib.lib()
    src = _aligned(img.size)
    src[:] = img
    out = _aligned(L.lqer_weight_narrow_bytes(N, K, C.byref(f)))
    rc = L.lqer_weight_narrow_host(src.ctypes.data, N, K, C.byref(f), out.ctypes.data)
    return rc, out


def _widen_host(nar, N, K, f):
    L = _lib.lib()
    Np, Kp = R.padded(N, K)
    src = _aligned(nar.size)
    src[:] = nar
    out = _aligned((Np // 16) * (Kp // 64) * R.STD_PANEL)
    out[:] = 0xA5  # (every byte of the standard image must be written)
    _lib.check(L.lqer_weight_widen_host(src.ctypes.data, N, K, C.byref(f), out.ctypes.data), "lqer_weight_widen_host")
    return out


def test_abi_version_and_new_symbols():
    L = _lib.lib()
    assert L.lqer_version() == 14 and _lib.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "lqer_hip.h")).read()
    assert re.search(r"#define LQER_ABI_VERSION 14\b", header)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        getattr(L, name)
    assert L.lqer_sizeof_linear_desc() == C.sizeof(LinearDesc) and L.lqer_sizeof_group_member() == C.sizeof(_lib.GroupMember)


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("width,block", FORMATS)
def test_narrow_bytes_formula(width, block, N, K):
    Np, Kp = R.padded(N, K)
    E = R.exps_per_row(width, block, K)
    assert E == {(2, 16): 4, (2, 32): 2, (3, 32): 2, (3, 16): 4, (3, 128): 1, (2, -1): 1, (3, 48): 4}[(width, block)]
    got = _lib.lib().lqer_weight_narrow_bytes(N, K, C.byref(_wfmt(width, block)))
    assert got == (Np // 16) * (Kp // 64) * (128 * width + 16 * E)


def test_narrow_bytes_is_zero_for_formats_that_are_not_served():
    L = _lib.lib()
    for f in (_wfmt(4, 16), _wfmt(8, -1), _wfmt(5, 16), _wfmt(3, 16, _lib.Q_INT), _wfmt(2, 16, _lib.Q_INT),
              QFmt(_lib.Q_MINIFLOAT, 3, -1, 1, 1), QFmt(_lib.Q_MINIFLOAT, 4, -1, 2, 1), _wfmt(3, 16, _lib.Q_PASSTHROUGH)):
        assert L.lqer_weight_narrow_bytes(48, 200, C.byref(f)) == 0, (f.kind, f.width)
    assert L.lqer_weight_narrow_bytes(48, 200, None) == 0


@pytest.mark.parametrize("width,block", FORMATS)
def test_host_round_trip_is_byte_exact(width, block):
    N, K = 48, 200
    f = _wfmt(width, block)
    img = R.random_std_image(N, K, width, block, seed=100 * width + block)
    rc, nar = _narrow_host(img, N, K, f)
    assert rc == 0, _lib.lib().lqer_last_error()
    back = _widen_host(nar, N, K, f)
    assert np.array_equal(back, img)
    # ... and the compact bytes are the ones the header describes: every code and every exponent byte, read back one by one
    Np, Kp = R.padded(N, K)
    E = R.exps_per_row(width, block, K)
    pb = R.panel_bytes(width, E)
    std = img.reshape(-1, R.STD_PANEL)
    cmp_ = nar.reshape(-1, pb)
    for p in (0, 3, 4 * (Np // 16) - 1):  # first panel, the panel that K = 200 cuts, the last panel (rows past N)
        for row in range(16):
            for k in range(64):
                assert R.narrow_code(cmp_[p], width, row, k) == R.std_code(std[p], row, k), (p, row, k)
            for seg in range(4):
                live = (p % (Kp // 64)) * 64 + seg * 16 < K
                if live or E == 4:
                    assert R.narrow_exp(cmp_[p], width, E, row, seg) == R.std_exp(std[p], row, seg), (p, row, seg)


def test_host_narrow_refuses_bytes_that_are_not_such_an_image():
    N, K = 48, 200
    f = _wfmt(2, 32)
    img = R.random_std_image(N, K, 2, 32, seed=1)
    bad = img.copy()
    bad[0] |= 0x02  # a second magnitude bit in a width-2 image
    assert _narrow_host(bad, N, K, f)[0] == -1
    bad = img.copy()
    bad[512 + 1] ^= 0x10  # the two exponent bytes of one block of 32 differ
    assert _narrow_host(bad, N, K, f)[0] == -1
    assert b"widening would not give it back" in _lib.lib().lqer_last_error()


@pytest.mark.parametrize("block", [16, 32, 128])
def test_width3_fields_do_not_bleed(block):
    """Every code field takes each of its 8 values (over 8 images, its neighbours holding other values) and every exponent byte of a
    panel a value of its own; the compact image is read back field by field."""
    N, K, width = 16, 128, 3
    f = _wfmt(width, block)
    Np, Kp = R.padded(N, K)
    E = R.exps_per_row(width, block, K)
    pb = R.panel_bytes(width, E)
    npanels = (Np // 16) * (Kp // 64)
    rows = np.arange(16).reshape(16, 1)
    ks = np.arange(64).reshape(1, 64)
    for shift in range(8):
        img = np.zeros((npanels, R.STD_PANEL), dtype=np.uint8)
        for p in range(npanels):
            val = (5 * (64 * rows + ks) + 3 * p + shift) % 8  # sign << 2 | magnitude of (row, k): each of the 8 values over the shifts
            for row in range(16):
                for k in range(64):
                    v = int(val[row, k])
                    nib = (v >> 2) << 3 | (v & 3)
                    c, j8 = k // 8, k % 8
                    off = row * 32 + (c & 1) * 16 + (c >> 1) * 4
                    pos = 2 * j8 if j8 < 4 else 2 * (j8 - 4) + 1
                    img[p, off + pos // 2] |= nib << (4 * (pos & 1))
                for seg in range(4):
                    img[p, 512 + row * 4 + seg] = 1 + (37 * p + 4 * row + seg * E // 4 + 11 * shift) % 254  # distinct per compact byte
        rc, nar = _narrow_host(img.reshape(-1), N, K, f)
        assert rc == 0, _lib.lib().lqer_last_error()
        cmp_ = nar.reshape(npanels, pb)
        for p in (0, 1, npanels - 1):
            for row in range(16):
                for k in range(64):
                    v = (5 * (64 * row + k) + 3 * p + shift) % 8
                    assert R.narrow_code(cmp_[p], width, row, k) == (v >> 2, v & 3), (shift, p, row, k)
                for seg in range(4):
                    assert R.narrow_exp(cmp_[p], width, E, row, seg) == int(img[p, 512 + row * 4 + seg]), (shift, p, row, seg)
        assert np.array_equal(_widen_host(nar, N, K, f), img.reshape(-1))


def _desc(x, w, rank=32, tuning=0, K=512, N=256):
    mx8 = QFmt(_lib.Q_MXINT, 8, 16, 8, 127)
    return LinearDesc(K, N, rank, 0, x, w, QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127), mx8, mx8, tuning)


def test_host_side_refusals_name_their_reason():
    L = _lib.lib()
    mx8 = QFmt(_lib.Q_MXINT, 8, 16, 8, 127)
    cases = {
        "int8": _desc(QFmt(_lib.Q_MXINT_I8, 8, -1, 8, 127), _wfmt(2, 128)),
        "limb": _desc(QFmt(_lib.Q_PASSTHROUGH, 24, 0, 8, 127), _wfmt(3, 32)),
        "width 4": _desc(mx8, _wfmt(4, 16)),
        "integer": _desc(mx8, QFmt(_lib.Q_INT, 3, -1, 1, 2)),
        "LQER_TUNE_W_EXP_TABLE": _desc(mx8, _wfmt(3, 16), tuning=_lib.TUNE_W_EXP_TABLE),
    }
    for what, d in cases.items():
        for M in (1, 300):
            assert L.lqer_weight_narrow_route(C.byref(d), M, _lib.F32, 512, 1, 1) == -2, what
            msg = L.lqer_last_error().decode()
            assert "compact weight image" in msg and len(msg) > 30, (what, msg)
        assert L.lqer_linear_forward_narrow_workspace_bytes(C.byref(d), 300) == 0, what
    assert "int8" in (L.lqer_weight_narrow_route(C.byref(cases["int8"]), 1, _lib.F16, 512, 1, 1), L.lqer_last_error().decode())[1]
    assert "limb" in (L.lqer_weight_narrow_route(C.byref(cases["limb"]), 1, _lib.F32, 512, 1, 1), L.lqer_last_error().decode())[1]
    assert "width 4" in (L.lqer_weight_narrow_route(C.byref(cases["width 4"]), 1, _lib.F16, 512, 1, 1), L.lqer_last_error().decode())[1]


def test_route_query_and_workspace_of_a_served_descriptor():
    L = _lib.lib()
    mx8 = QFmt(_lib.Q_MXINT, 8, 16, 8, 127)
    d = _desc(mx8, _wfmt(2, 16))
    sz = _lib.LinearSizes()
    for M, want in ((1, _lib.NARROW_DIRECT_ONE_LAUNCH), (8, _lib.NARROW_DIRECT_ONE_LAUNCH), (9, _lib.NARROW_DIRECT), (64, _lib.NARROW_DIRECT),
                    (65, _lib.NARROW_WIDEN), (300, _lib.NARROW_WIDEN)):
        assert L.lqer_weight_narrow_route(C.byref(d), M, _lib.F16, 512, 1, 1) == want, M
        assert L.lqer_linear_sizes(C.byref(d), M, C.byref(sz)) == 0
        need = L.lqer_linear_forward_narrow_workspace_bytes(C.byref(d), M)
        image = (256 // 16) * (512 // 64) * 576
        assert need == (sz.workspace if M <= 64 else (sz.workspace + 255) // 256 * 256 + image), M
    # a row stride that is not a multiple of 16 bytes, or two limbs of A: the two-launch route, still direct
    assert L.lqer_weight_narrow_route(C.byref(d), 7, _lib.F16, 513, 1, 1) == _lib.NARROW_DIRECT
    assert L.lqer_weight_narrow_route(C.byref(d), 7, _lib.F16, 512, 2, 1) == _lib.NARROW_DIRECT
    # B_out with one block per row sends decode sizes to the tile kernel: widened at every M
    d2 = _desc(mx8, _wfmt(2, -1))
    d2.b_out_fmt = QFmt(_lib.Q_MXINT, 8, -1, 8, 127)
    assert L.lqer_weight_narrow_route(C.byref(d2), 3, _lib.F16, 512, 1, 1) == _lib.NARROW_WIDEN
    assert L.lqer_linear_forward_narrow_workspace_bytes(C.byref(d2), 3) > ops_workspace(d2, 3)


def ops_workspace(d, M):
    sz = _lib.LinearSizes()
    assert _lib.lib().lqer_linear_sizes(C.byref(d), M, C.byref(sz)) == 0
    return sz.workspace

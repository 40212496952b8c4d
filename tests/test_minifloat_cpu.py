"""The reference's `minifloat` quantizer on the host side: format descriptors per role, the refusals, the test-local statement
(tests/_minifloat.py) against the reference's own outputs, and LQER_Q_MINIFLOAT / ABI 14 across the header, the binding and the .so."""
import os
import re

import numpy as np
import pytest
import torch

import _minifloat as MF
from lqer_amd import _lib, ops

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "minifloat.npz"))
KEYS = sorted({k.split("/")[0] for k in GOLD.files})


def mf(w, ew, eb=None):
    return dict(name="minifloat", width=w, exponent_width=ew, exponent_bias=eb)


@pytest.mark.parametrize("role", ["x", "w", "b", "A_out", "B_out"])
def test_make_qfmt_fields(role):
    f = ops.make_qfmt(mf(4, 2, 7), role)
    assert (f.kind, f.width, f.block, f.exp_width, f.exp_bias) == (_lib.Q_MINIFLOAT, 4, -1, 2, 7)
    assert not hasattr(f, "act_tiles") and not hasattr(f, "block_rows")
    for eb in (None, "none", "None", "NA"):  # the reference's default bias 2^(ew-1) - 1
        assert ops.make_qfmt(mf(4, 2, eb), role).exp_bias == 1
    if role != "w":
        g = ops.make_qfmt(mf(8, 4, 7), role)
        assert (g.width, g.exp_width, g.exp_bias) == (8, 4, 7)
        assert ops.make_qfmt(mf(8, 5), role).exp_bias == 15


def test_make_qfmt_refusals():
    with pytest.raises(NotImplementedError):  # no exponent_width: names no format (as test_abi_cpu asserts too)
        ops.make_qfmt(dict(name="minifloat", width=8))
    with pytest.raises(ValueError):  # mbits = width - exponent_width - 1 < 0
        ops.make_qfmt(mf(4, 4))
    with pytest.raises(ValueError):
        ops.make_qfmt(mf(9, 4))
    with pytest.raises(NotImplementedError):  # values beyond the normal bf16 range
        ops.make_qfmt(mf(8, 4, 140))
    with pytest.raises(NotImplementedError):
        ops.make_qfmt(mf(8, 5, -120))
    for w in (5, 6, 8):  # minifloat weights need a 4-bit code
        with pytest.raises(NotImplementedError):
            ops.make_qfmt(mf(w, 3), "w")
    assert ops.make_qfmt(mf(8, 4, 7), "x").kind == _lib.Q_MINIFLOAT


@pytest.mark.parametrize("key", KEYS)
def test_statement_matches_reference(key):
    w, ew, b = (int(v) for v in GOLD[f"{key}/fmt"])
    x, y = torch.from_numpy(GOLD[f"{key}/x"]), torch.from_numpy(GOLD[f"{key}/y"])
    got = MF.minifloat(x, w, ew, b)
    assert torch.equal(got, y), int((got != y).sum())
    assert torch.equal(torch.signbit(got), torch.signbit(y))
    # fp16 inputs evaluated in fp32 (this project's convention) against the same values in fp32
    x16 = torch.from_numpy(GOLD[f"{key}/x16"])
    assert torch.equal(MF.minifloat(x16.float(), w, ew, b), torch.from_numpy(GOLD[f"{key}/y16_fp32"]))
    # the declared divergence: the reference evaluating in fp16 differs on this many elements (fp16 log2 / arithmetic)
    n = int((torch.from_numpy(GOLD[f"{key}/y16_ref"]) != torch.from_numpy(GOLD[f"{key}/y16_fp32"])).sum())
    assert n == int(GOLD[f"{key}/n_fp16_diff"][0])


def test_floor_log2_rounding_pinned():
    # torch's fp32 log2 lifts 256 (1 - 2^-24) to 8: (8, 4, 7) quantizes it to 256, not 240
    x = torch.tensor([256 * (1 - 2**-24), 256 * (1 - 2**-23)], dtype=torch.float32)
    assert MF.minifloat(x, 8, 4, 7).tolist() == [256.0, 256.0]
    assert float(MF.minifloat(torch.tensor([1000.0]), 8, 4, 7)) == 480.0  # saturation
    assert MF.values(8, 4, 7).max().item() == 480.0


def _header():
    with open(os.path.join(HERE, "..", "include", "lqer_hip.h")) as fh:
        return fh.read()


def test_abi14_header_binding():
    h = _header()
    assert int(re.search(r"#define LQER_ABI_VERSION (\d+)", h).group(1)) == 14 == _lib.ABI_VERSION
    assert int(re.search(r"#define LQER_Q_MINIFLOAT (\d+)", h).group(1)) == _lib.Q_MINIFLOAT == 5


def test_abi14_library():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("liblqer_hip.so not built")
    L = _lib.lib()
    assert L.lqer_version() == 14


def _floor_log2_rule(v: np.ndarray) -> np.ndarray:
    """common.h floor_log2_rule, restated on fp32 bit patterns (v > 0, normal)."""
    bits = v.astype(np.float32).view(np.uint32).astype(np.int64)
    kl = ((bits >> 23) & 0xFF) - 127
    d = (1 << 23) - (bits & 0x7FFFFF)
    K = kl + 1
    aK = np.abs(K)
    q = np.floor(np.log2(np.maximum(aK, 1))).astype(np.int64) - ((K > 0) & ((K & (K - 1)) == 0)).astype(np.int64)
    slack = np.where((K == 0) | (q < 0), 0, np.floor(np.ldexp(np.float32(0.6931472), np.maximum(q, 0))).astype(np.int64))
    return np.where(d <= slack, K, kl)


def test_floor_log2_rule_against_torch():
    # every exponent of normal fp32 numbers, d = 1..120 ulps below each power of two (the rule's boundary is at most 44), and a
    # random sample of mantissas: the bit rule the kernels use is torch.floor(torch.log2(v)) in fp32
    K = np.arange(-125, 128)
    d = np.arange(1, 121)
    v = (np.ldexp(1.0, K)[:, None] * (1 - d[None, :] * 2.0**-24)).astype(np.float32).ravel()
    rng = np.random.default_rng(0)
    r = np.ldexp(rng.uniform(1.0, 2.0, 20000), rng.integers(-126, 127, 20000)).astype(np.float32)
    for t in (v, r):
        want = torch.floor(torch.log2(torch.from_numpy(t))).numpy().astype(np.int64)
        assert np.array_equal(_floor_log2_rule(t), want)

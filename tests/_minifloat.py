"""Test-local CPU statement of the reference's `minifloat` quantizer (quantizers/minifloat.py:120-182, `minifloat_ieee`, what
get_quantizer("minifloat") returns) and of a Linear forward that uses it in any role.  `oracle/` stays as it is (its get_quantizer
refuses minifloat); this module is pinned bit for bit to the reference's own outputs in tests/golden/minifloat.npz by
tests/test_minifloat_cpu.py.  Evaluated in fp32: a fp16 / bf16 input is upcast first."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from oracle import lqer_oracle as O


def resolve_bias(exponent_width: int, exponent_bias=None) -> int:
    """The reference's default bias 2^(exponent_width - 1) - 1 for None / "none" / "None" / "NA"."""
    if exponent_bias in (None, "none", "None", "NA"):
        return 2 ** (exponent_width - 1) - 1
    return int(exponent_bias)


def minifloat(x: torch.Tensor, width: int, exponent_width: int, exponent_bias=None) -> torch.Tensor:
    """sign(x) 2^e (1 + S 2^-m) for normal values, sign(x) 2^(e+1) S 2^-m in the lowest binade (e = -bias), with
    e = clamp(floor(log2(|x| + 1e-9)), -bias, 2^ew - 1 - bias) - torch's fp32 log2, whose rounding lifts values a few ulps below a
    power of two to that power -, S the round-half-even mantissa field clamped to [0, 2^m - 1] (a value never rounds into the next
    binade); |x| <= 1e-8 is returned unchanged."""
    x = x.to(torch.float32)
    m = width - exponent_width - 1
    bias = resolve_bias(exponent_width, exponent_bias)
    lo, hi = -bias, 2**exponent_width - 1 - bias
    a = x.abs()
    e = torch.floor(torch.log2(a + 1e-9)).clamp(lo, hi)
    p = torch.pow(2.0, e)  # exact: an integer exponent
    frac = a / p
    sub = e == lo
    s_norm = torch.round(frac * 2**m - 2**m).clamp(0, 2**m - 1)
    s_sub = torch.round(frac * 2**m / 2).clamp(0, 2**m - 1)
    mant = torch.where(sub, s_sub / 2**m * 2, 1.0 + s_norm / 2**m)
    v = torch.sign(x + 1e-9) * p * mant
    # (|x| <= 1e-8 comes back as 0 v + 1 x = x, where a -0 input becomes +0)
    return torch.where(a <= 1e-8, x + 0.0, v)


def values(width: int, exponent_width: int, exponent_bias=None) -> torch.Tensor:
    """Every non-negative value of the format, ascending (magnitude codes 0 .. 2^(width-1) - 1)."""
    m = width - exponent_width - 1
    bias = resolve_bias(exponent_width, exponent_bias)
    out = []
    for c in range(2 ** (width - 1)):
        E, S = c >> m, c & (2**m - 1)
        out.append(2.0 ** (1 - bias) * S / 2**m if E == 0 else 2.0 ** (E - bias) * (1 + S / 2**m))
    return torch.tensor(out, dtype=torch.float32)


def get_quantizer(cfg: Optional[dict]):
    """oracle.get_quantizer with `minifloat` added (quantizers/__init__.py:7-18)."""
    if cfg is not None and cfg.get("name") == "minifloat":
        w, ew, eb = int(cfg["width"]), int(cfg["exponent_width"]), cfg.get("exponent_bias")
        return lambda t: minifloat(t, w, ew, eb)
    return O.get_quantizer(cfg)


def linear_forward(x, weight, bias, A, B, q_config: dict, intermediates: bool = False):
    """y = Q_x(x) Q_w(W)^T + Q_b(b) + Q_Bout(Q_Aout(Q_x(x) A) B) in fp32 (reference linear.py:145-157; A = None: LinearFlexible),
    with the reference's fall-back of A_out / B_out to x's config (linear.py:115-124)."""
    qs = O.resolve_linear_quantizers(q_config)
    xq = get_quantizer(qs["x"])(x.to(torch.float32))
    wq = get_quantizer(qs["w"])(weight.to(torch.float32))
    bq = None if bias is None else get_quantizer(qs["b"])(bias.to(torch.float32))
    y = F.linear(xq, wq, bq)
    out = {"xq": xq, "wq": wq}
    if A is not None:
        xAq = get_quantizer(qs["A_out"])(torch.matmul(xq, A.to(torch.float32)))
        y = y + get_quantizer(qs["B_out"])(torch.matmul(xAq, B.to(torch.float32)))
        out["xAq"] = xAq
    out["y"] = y
    return out if intermediates else y


def envelope_bad(s64, got, width: int, exponent_width: int, exponent_bias, D: float) -> int:
    """A minifloat A_out of an fp32 sum taken in another order than the reference's (xAq = A_out(xq @ A)): every product is exact,
    so any order lands within D ulps of the exact sum s; the quantizer is monotone, so each entry of the bf16 image must lie between
    the images of s - D ulp and s + D ulp (|v| <= 1e-8 flushed to 0 in the image).  Returns the number of entries outside."""
    import numpy as np

    s64 = np.asarray(s64, dtype=np.float64)
    ulp = np.spacing(np.abs(s64).astype(np.float32)).astype(np.float64)
    lo = torch.from_numpy((s64 - D * ulp).astype(np.float32))
    hi = torch.from_numpy((s64 + D * ulp).astype(np.float32))
    qlo, qhi = minifloat(lo, width, exponent_width, exponent_bias), minifloat(hi, width, exponent_width, exponent_bias)
    flush = lambda q: torch.where(q.abs() <= 1e-8, torch.zeros_like(q), q)  # noqa: E731
    qlo, qhi = flush(qlo), flush(qhi)
    g = torch.as_tensor(np.asarray(got, dtype=np.float32))
    ok = (g >= torch.minimum(qlo, qhi)) & (g <= torch.maximum(qlo, qhi))
    ok |= (g == 0) & ((lo.abs() <= 1e-8) | (hi.abs() <= 1e-8) | (torch.sign(lo) != torch.sign(hi)))
    return int((~ok).sum())

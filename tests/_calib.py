"""Test-local float64 restatement of the reference's two calibration hook bodies (src/lqer/statistic_profiler/scale.py:32-51,
threshold.py:39-40, :53-79), the error bounds derived for them, and a torch CPU stand-in for ops.col_abs_stats (the factories' test
seam).  Pinned to the reference's own outputs in tests/golden/calib.npz by tests/test_calibrate_cpu.py."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24  # unit roundoff of fp32
CLAMP = float(np.float32(1e-4))  # the reference clamps an fp32 tensor: the constant as fp32 holds it


def scale_step(scale: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """one call of the scale hook in float64: max(scale, mean(|x|) per input channel)"""
    return torch.maximum(scale, x.double().abs().reshape(-1, x.shape[-1]).mean(0))


def normalise(scale: torch.Tensor) -> torch.Tensor:
    """get_scale_dict in float64: clamp(min = 1e-4), divide by sqrt(min * max)"""
    s = scale.double().clamp(min=CLAMP)
    return s / torch.sqrt(s.min() * s.max())


def n_cols_ge(x: torch.Tensor, threshold: float) -> int:
    """one call of the threshold hook: columns holding an |x| >= threshold (thresholds exactly representable in x's dtype)"""
    return int((x.double().abs() >= threshold).reshape(-1, x.shape[-1]).any(dim=0).sum())


def threshold_entry(counts, weight_shape, threshold, seq_len) -> dict:
    n = math.ceil(sum(counts) / len(counts))
    o, i = weight_shape
    return {"weight_shape": [o, i], "high_precision_weight_shape": [o, n], "low_precision_weight_shape": [o, i - n],
            "high_precision_activation_shape": [seq_len, n], "low_precision_activation_shape": [seq_len, i - n],
            "threshold": threshold, "seq_len": seq_len, "num_activation_columns_in_high_precision": n}


def as_lists(d):
    """tuples -> lists, recursively (what a JSON round trip does to the reference's dictionary)"""
    if isinstance(d, dict):
        return {k: as_lists(v) for k, v in d.items()}
    if isinstance(d, (tuple, list)):
        return [as_lists(v) for v in d]
    return d


# The bounds (derived, not measured): any order of summing M non-negative fp32 numbers is within (M - 1) u / (1 - (M - 1) u) of the
# exact sum relatively, the division adds u, max over batches preserves a relative bound -> a running scale within M u of float64,
# two fp32 evaluations within 2 M u of each other.  The normalisation multiplies by 1 / sqrt(min * max) (half the relative error of
# each factor) and rounds a few more times: 2 M u + 8 u against float64, twice that between two fp32 evaluations.
def bound_scale(M: int, vs_ref: bool) -> float:
    return (2 if vs_ref else 1) * M * U


def bound_norm(M: int, vs_ref: bool) -> float:
    return (2 if vs_ref else 1) * (2 * M * U + 8 * U)


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """largest |got - want| / |want| (0 where both are 0; inf where only `want` is)"""
    g, w = got.double().cpu(), want.double().cpu()
    d = (g - w).abs()
    r = torch.where(w != 0, d / w.abs(), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return float(r.max())


def stats_cpu(x: torch.Tensor, run=None, want_absmax: bool = False, threshold=None):
    """torch stand-in for ops.col_abs_stats on CPU tensors (fp32 arithmetic, as the reference hook)"""
    from lqer_amd.ops import ColStats

    xf = x.float().abs().reshape(-1, x.shape[-1])
    if run is None and not want_absmax and threshold is None:
        run = torch.zeros(x.shape[-1])
    if run is not None:
        run.copy_(torch.maximum(run, xf.mean(0)))
    absmax = xf.amax(0) if want_absmax else None
    count = (xf >= threshold).any(0).sum().to(torch.int32).reshape(1) if threshold is not None else None
    return ColStats(run, absmax, count)


def load_fixture():
    g = np.load(os.path.join(HERE, "golden", "calib.npz"))
    with open(os.path.join(HERE, "golden", "calib.json")) as fh:
        meta = json.load(fh)
    return g, meta


def case_batches(g, meta, name):
    """the case's input batches as the reference was handed them (fp32 cases whose values are fp16 numbers are stored as fp16)"""
    c = meta["cases"][name]
    dt = getattr(torch, c["dtype"])
    return [torch.from_numpy(g[f"{name}/x{b}"]).to(dt).reshape(c["shape"]) for b in range(c["batches"])]

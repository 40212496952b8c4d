"""Calibration profiler: the producer of L2QER's `scale_dict` and of the outlier-column counts, on the HIP path.

Counterpart of the reference's `lqer.statistic_profiler` (src/lqer/statistic_profiler/scale.py, threshold.py) and of the hook part of
`run_profiler` (src/lqer/runners.py:55-121): forward hooks on every nn.Linear record, per input channel, the running maximum over
calibration batches of mean(|x|) - normalised once at the end - or count the columns that hold an |x| >= threshold.  Same class and
function names, same `scales` / `results` / `is_profiled` attributes, same dictionary keys ("<module name>.scale",
"<module name>.threshold"), so `approximate.approximate_model(..., scale_dict=...)` and the reference's `load_scale_dict`
(lqer_act.py:153-159) read the result alike.

The hook body is one call of `ops.col_abs_stats` (csrc/col_stats.hip: one pass over x in its own dtype instead of an fp32 copy, an abs
copy and a column mean); the normalisation is a [K] torch expression run once.  Counts stay on the device until `get_threshold_dict()`
(the reference's `.item()` per hook call is a host synchronisation per Linear).  There is no CPU path: without `stats_fn` (a test seam
like approximate_model's `factors_fn`) a CPU tensor raises what every op of this package raises.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional

import torch
import torch.nn as nn

from . import ops

SCALE_CLAMP_MIN = 1e-4


class ScaleHookFactoryBase:
    def __init__(self, stats_fn: Optional[Callable] = None):
        self.scales: Dict[str, torch.Tensor] = {}
        self.is_profiled: Dict[str, bool] = {}
        self.handles = []  # what register_scale_hooks registered (profile_model removes them)
        self._stats = stats_fn or ops.col_abs_stats

    def get_scale_hook(self, name: str, in_features: int) -> Callable:
        raise NotImplementedError("get_scale_hook is not implemented.")

    def is_all_profiled(self) -> bool:
        return all(self.is_profiled.values())

    def get_scale_dict(self) -> Dict[str, torch.Tensor]:
        raise NotImplementedError("get_scale_dict is not implemented.")

    def remove_hooks(self) -> None:
        for h in self.handles:
            h.remove()
        self.handles = []


class ScaleHookFactoryMeanAbs(ScaleHookFactoryBase):
    def get_scale_hook(self, name: str, in_features: int) -> Callable:
        self.scales[name] = torch.zeros(in_features, dtype=torch.float32)
        self.is_profiled[name] = False

        @torch.no_grad()
        def scale_hook(module: nn.Linear, input, output) -> None:
            x = input[0]
            scale = self.scales[name]
            if scale.device != x.device:  # (the running scale lives where the input lives: first call, or a re-dispatched model)
                scale = scale.to(x.device)
            # scale = max(scale, mean(|x|) per input channel), in place (scale.py:32-38)
            self.scales[name] = self._stats(x, run=scale).run
            self.is_profiled[name] = True

        return scale_hook

    def get_scale_dict(self) -> Dict[str, torch.Tensor]:
        assert self.is_all_profiled(), "Not all scales are profiled."
        for name, scale in self.scales.items():
            scale = scale.clamp(min=SCALE_CLAMP_MIN)
            scale = scale / torch.sqrt(scale.min() * scale.max())
            self.scales[name] = scale
        return self.scales


def register_scale_hooks(model: nn.Module, mode: str = "mean(abs())", stats_fn: Optional[Callable] = None) -> ScaleHookFactoryMeanAbs:
    """A scale hook on every nn.Linear of `model` (subclasses included: a model after quantize_model works too), keyed
    "<module name>.scale" (scale.py:54-69)."""
    if mode == "mean(abs())":
        factory = ScaleHookFactoryMeanAbs(stats_fn)
    else:
        raise ValueError(f"Unknown mode: {mode}")
    for name, module in model.named_modules():
        if not isinstance(module, nn.Linear):
            continue
        factory.handles.append(module.register_forward_hook(factory.get_scale_hook(name + ".scale", module.in_features)))
    return factory


class ThresholdHookFactory:
    def __init__(self, threshold: float, seq_len: int, stats_fn: Optional[Callable] = None):
        self.threshold = threshold
        self.seq_len = seq_len
        self.results: Dict[str, dict] = {}
        self.is_profiled: Dict[str, bool] = {}
        self.handles = []
        self._stats = stats_fn or ops.col_abs_stats

    def get_threshold_hook(self, name: str, in_features: int, out_features: int) -> Callable:
        self.results[name] = {
            "weight_shape": (out_features, in_features),
            "high_precision_weight_shape": None,
            "low_precision_weight_shape": None,
            "high_precision_activation_shape": None,
            "low_precision_activation_shape": None,
            "running_num_x_cols_hp": None,
        }
        self.is_profiled[name] = False

        @torch.no_grad()
        def threshold_hook(module: nn.Linear, input, output) -> None:
            x = input[0]
            assert x.ndim >= 2
            # columns with some |x| >= threshold (threshold.py:39-40); the count stays on the device
            count = self._stats(x, threshold=self.threshold).count
            if self.results[name]["running_num_x_cols_hp"] is None:
                self.results[name]["running_num_x_cols_hp"] = [count]
            else:
                self.results[name]["running_num_x_cols_hp"].append(count)
            self.is_profiled[name] = True

        return threshold_hook

    def is_all_profiled(self) -> bool:
        return all(self.is_profiled.values())

    def get_threshold_dict(self) -> Dict[str, dict]:
        assert self.is_all_profiled(), "Not all thresholds are profiled."
        # every per-call count of every module in one read per device
        cells = [(name, c) for name, r in self.results.items() for c in r["running_num_x_cols_hp"]]
        host: Dict[str, list] = {name: [] for name in self.results}
        by_dev: Dict[torch.device, list] = {}
        for name, c in cells:
            by_dev.setdefault(c.device, []).append((name, c))
        for group in by_dev.values():
            vals = torch.cat([c.reshape(1) for _, c in group]).tolist()
            for (name, _), v in zip(group, vals):
                host[name].append(int(v))
        for name, result in self.results.items():
            result.pop("running_num_x_cols_hp")
            reduced_x = host[name]
            x_n_cols_hp = math.ceil(sum(reduced_x) / len(reduced_x))
            w_shape = result["weight_shape"]
            result["high_precision_weight_shape"] = (w_shape[0], x_n_cols_hp)
            result["low_precision_weight_shape"] = (w_shape[0], w_shape[1] - x_n_cols_hp)
            result["high_precision_activation_shape"] = (self.seq_len, x_n_cols_hp)
            result["low_precision_activation_shape"] = (self.seq_len, w_shape[1] - x_n_cols_hp)
            result["threshold"] = self.threshold
            result["seq_len"] = self.seq_len
            result["num_activation_columns_in_high_precision"] = x_n_cols_hp
        return self.results

    def remove_hooks(self) -> None:
        for h in self.handles:
            h.remove()
        self.handles = []


def register_threshold_hooks(model: nn.Module, threshold: float, seq_len: int, stats_fn: Optional[Callable] = None) -> ThresholdHookFactory:
    """A threshold hook on every nn.Linear of `model`, keyed "<module name>.threshold" (threshold.py:82-96)."""
    factory = ThresholdHookFactory(threshold, seq_len=seq_len, stats_fn=stats_fn)
    for name, module in model.named_modules():
        if not isinstance(module, nn.Linear):
            continue
        factory.handles.append(module.register_forward_hook(
            factory.get_threshold_hook(name + ".threshold", module.in_features, module.out_features)))
    return factory


@torch.no_grad()
def profile_model(model: nn.Module, batches: Iterable, mode: str = "mean(abs())", stats_fn: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    """The hook part of the reference's run_profiler (runners.py:80-113): register the scale hooks, run the model over `batches` (each a
    dict -> model(**batch), a tuple / list -> model(*batch), anything else -> model(batch)), remove the hooks and return the normalised
    scales as CPU tensors - what the reference saves as scale_dict.pt.  Datasets and tokenizers are the caller's business."""
    factory = register_scale_hooks(model, mode, stats_fn)
    try:
        for batch in batches:
            if isinstance(batch, dict):
                model(**batch)
            elif isinstance(batch, (tuple, list)):
                model(*batch)
            else:
                model(batch)
    finally:
        factory.remove_hooks()
    return {k: v.cpu() for k, v in factory.get_scale_dict().items()}

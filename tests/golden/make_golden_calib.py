"""Generate the calibration golden vectors under tests/golden/ by importing the REFERENCE (read-only, at /root/reference) in the build
container, with make_golden.py's recipe.  Run once, here:  python tests/golden/make_golden_calib.py

The closures of the reference's get_scale_hook / get_threshold_hook are called directly with (None, (x,), None) over 3 batches per
case.  Only data is written: calib.npz (inputs, `factory.scales` before the normalisation, get_scale_dict() after it) and calib.json
(case descriptions and the threshold dictionaries).  The tests that read them never touch the reference.
"""
import json
import os
import zlib

import numpy as np
import torch

from make_golden import HERE, import_reference

# name, dtype of the tensor handed to the hooks, shape of one batch, thresholds, stored as fp16 (fp32 inputs whose values are fp16 numbers)
CASES = [
    ("f32_2d_k50_m1", "float32", (1, 50), False),
    ("f32_3d_k100_m37", "float32", (1, 37, 100), False),
    ("f16_2d_k768_m37", "float16", (37, 768), False),
    ("f16_3d_k50_m1000", "float16", (4, 250, 50), False),
    ("f32_2d_k768_m1", "float32", (1, 768), False),
    ("f16_2d_k100_m37", "float16", (37, 100), False),
    ("f32_3d_k50_m1000", "float32", (2, 500, 50), True),
]
THRESHOLDS = (6.0, 0.5)
SEQ_LEN = 128
OUT_FEATURES = 24


def make_batches(name, dtype, shape):
    torch.manual_seed(zlib.crc32(name.encode()) % 10000)
    K = shape[-1]
    out = []
    for b in range(3):
        x = torch.randn(*shape)
        col = torch.ones(K)
        col[[3, K // 2, K - 2]] = 50.0        # outlier columns, 50x the rest
        col[K - 1] = 1e-5                      # a column that stays below the clamp
        col[5 + b] *= 4.0 + b                  # per-column maxima that come from different batches
        col[11] = 0.05                         # a column below the 0.5 threshold in most rows
        x = x * col
        out.append(x.to(getattr(torch, dtype)))
    return out


def main():
    import_reference()
    from lqer.statistic_profiler.scale import ScaleHookFactoryMeanAbs
    from lqer.statistic_profiler.threshold import ThresholdHookFactory

    g, meta = {}, {"thresholds": list(THRESHOLDS), "seq_len": SEQ_LEN, "out_features": OUT_FEATURES, "cases": {}}
    for name, dtype, shape, as_f16 in CASES:
        xs = make_batches(name, dtype, shape)
        if as_f16:  # an fp32 tensor whose values are fp16 numbers: stored in half the bytes, handed over as fp32
            xs = [x.half().float() for x in xs]
        K = shape[-1]
        key = "lin.scale"
        fac = ScaleHookFactoryMeanAbs()
        hook = fac.get_scale_hook(key, K)
        for x in xs:
            hook(None, (x,), None)
        g[f"{name}/scales"] = fac.scales[key].clone().numpy()
        g[f"{name}/scale_dict"] = fac.get_scale_dict()[key].clone().numpy()
        thr = {}
        for t in THRESHOLDS:
            tf = ThresholdHookFactory(t, seq_len=SEQ_LEN)
            th = tf.get_threshold_hook("lin.threshold", K, OUT_FEATURES)
            counts = []
            for x in xs:
                th(None, (x,), None)
                counts.append(tf.results["lin.threshold"]["running_num_x_cols_hp"][-1])
            thr[str(t)] = {"counts": counts, "dict": tf.get_threshold_dict()}
        for b, x in enumerate(xs):
            g[f"{name}/x{b}"] = (x.half() if as_f16 else x).numpy().reshape(-1)
        meta["cases"][name] = {"dtype": dtype, "shape": list(shape), "batches": len(xs), "rows": int(np.prod(shape[:-1])),
                               "stored_as_f16": as_f16, "thresholds": thr}
    np.savez_compressed(os.path.join(HERE, "calib.npz"), **g)
    with open(os.path.join(HERE, "calib.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print("calib.npz:", len(g), "arrays,", os.path.getsize(os.path.join(HERE, "calib.npz")), "bytes")


if __name__ == "__main__":
    main()

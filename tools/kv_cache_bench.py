"""Time a decode step's attention over the packed KV cache (lqer_amd.kvcache: lqer_kv_cache_append + lqer_attention_q_decode_kv)
against the decode kernel on the raw K and V (lqer_attention_q_decode), in this process on the same box, with HIP events.

    python tools/kv_cache_bench.py [--steps 200] [--warmup 10] [--rounds 5] [--out profiles/kv_cache.json]

Per shape [b, h, h_kv, s, t, d] of tools/attn_decode_bench.py (fp16, no mask: a decode step sees every key), legs on the same values,
alternating over several rounds with every round reported:
 (1) raw     attention_flexible(q, k, v, ..., kernel="decode"): K and V [.., t, d] read in fp16 and quantized in the kernel;
 (2) packed  cache.append(the step's s new tokens) at length t - s, then attention_flexible_cached(q, cache): what a step with the
             packed cache costs, the append included;
 (3) append  the append of (2) alone.
`timed` and the buffer rotation are tools/attn_bench.py's: enough distinct q / k / v / caches that the Infinity Cache holds none of
them (the rotation is sized by the packed cache, the smaller of the two).  What is timed is a CALL as a user makes it, Python and
launches included: at batch 1 up to t = 4096 that host side is longer than the kernels, so those rows compare what a call costs.
Reported per leg: microseconds (median of the rounds) and every round; the bytes each leg's model reads and writes (K and V once -
in fp16, or as codes and exponents, 17/16 byte per element - plus q, out and the decode kernel's workspace traffic as
tools/attn_decode_bench.py counts it; the packed leg also the append's staging rows, new rows and rewritten block); the cache's bytes
against the raw K and V; and whether the two legs' outputs are the same bits.
The criterion: at the two shapes where the kernels, not the host side, dominate the raw leg - (8, 32, 32, 1, 2048, 128) and
(1, 32, 32, 1, 32768, 128) - the packed leg's MEDIAN must be below the raw leg's FASTEST SINGLE ROUND; `criterion_met` says so per
gated shape and the tool exits non-zero when it does not hold.  The other shapes are reported only.  Not part of bench.py.  Needs a
GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attn_bench import L3_BYTES, timed  # noqa: E402
from attn_decode_bench import SHAPES, model_bytes  # noqa: E402
from benchlib.workloads import HBM_PEAK_GBS  # noqa: E402
from lqer_amd import QuantizedKVCache, attention_flexible, attention_flexible_cached  # noqa: E402

GATED = [(8, 32, 32, 1, 2048, 128), (1, 32, 32, 1, 32768, 128)]
LEGS = ("raw", "packed", "append")


def packed_model_bytes(b, h, hk, s, t, d):
    """model_bytes with K and V as codes and exponents (17/16 byte per element), plus the append: the s new rows of K and V read in fp16,
    up to 15 staging rows read and s written, the open block's codes and exponents and the new V rows written."""
    kv_raw = 2 * b * hk * t * d * 2
    kv_packed = 2 * b * hk * t * d * 17 // 16
    append = b * hk * d * (2 * s * 2 + 15 * 2 + s * 2 + 16 + 1 + s * 17 // 16 + 1)
    return model_bytes(b, h, hk, s, t, d) - kv_raw + kv_packed + append


def one_shape(b, h, hk, s, t, d, cfg, a):
    dt = torch.float16
    cache_bytes = QuantizedKVCache(b, hk, d, cfg, cfg, dt, "cuda", capacity=t).nbytes
    per = b * h * s * d * 2 + cache_bytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // per)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(s + t + d)
    bufs = []
    for _ in range(nbuf):
        q, k, v = (torch.randn(b, hh, n, d, generator=g, device="cuda", dtype=dt) for hh, n in ((h, s), (hk, t), (hk, t)))
        cache = QuantizedKVCache(b, hk, d, cfg, cfg, dt, "cuda", capacity=t)
        cache.append(k[:, :, :t - s], v[:, :, :t - s])  # the past; the timed step appends the last s keys, again and again at this length
        bufs.append((q, k, v, cache))
    scaling, past = d ** -0.5, t - s
    assert t % 16 == 0 and s < 16  # (the new keys stay inside the open block: such an append can be repeated at the same length)

    def append(q, k, v, cache):
        cache.length = past
        cache.append(k[:, :, past:], v[:, :, past:])

    def packed(q, k, v, cache):
        append(q, k, v, cache)
        return attention_flexible_cached(q, cache, scaling, out_layout="bshd")

    fns = {"raw": lambda q, k, v, cache: attention_flexible(q, k, v, cfg, cfg, scaling, out_layout="bshd", kernel="decode"), "packed": packed,
           "append": append}
    same = bool(torch.equal(fns["raw"](*bufs[0]), fns["packed"](*bufs[0])))
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    nbytes = {"raw": model_bytes(b, h, hk, s, t, d), "packed": packed_model_bytes(b, h, hk, s, t, d)}
    out = {"shape_b_h_hkv_s_t_d": [b, h, hk, s, t, d], "dtype": "float16", "buffers": nbuf, "same_bits": same, "cache_bytes": cache_bytes,
           "raw_kv_bytes": 2 * b * hk * t * d * 2, "gated": (b, h, hk, s, t, d) in GATED}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    for leg in ("raw", "packed"):
        gbs = nbytes[leg] / (med[leg] * 1e-6) / 1e9
        out[f"model_bytes_{leg}"] = nbytes[leg]
        out[f"gb_s_{leg}"] = round(gbs, 1)
        out[f"frac_of_hbm_peak_{leg}"] = round(gbs / HBM_PEAK_GBS, 4)
    out["speedup_packed_vs_raw"] = round(med["raw"] / med["packed"], 2)
    out["criterion_met"] = bool(med["packed"] < min(rounds["raw"])) if out["gated"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_cache.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_cache_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    with torch.no_grad():
        shapes = [one_shape(*sh, cfg, a) for sh in SHAPES]
    ok = all(s["criterion_met"] for s in shapes if s["gated"]) and all(s["same_bits"] for s in shapes)
    out = {"tool": "tools/kv_cache_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "steps": a.steps, "rounds": a.rounds, "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call included",
           "criterion": "at the gated shapes the packed leg's median (append included) below the fastest single round of the raw leg; the two "
                        "legs' outputs the same bits at every shape",
           "criterion_met": ok, "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the packed leg does not meet the criterion at a gated shape (or its output differs from the raw leg's)")


if __name__ == "__main__":
    main()

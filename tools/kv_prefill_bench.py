"""Time a chunk of a prompt attending over the packed KV cache with the prefill kernel (lqer_amd.kvcache: lqer_attention_q_kv - the two
bf16 images written from the cache's codes, then k_attn_q) against the same kernel on the raw K and V (lqer_attention_q, which
quantizes them into those images), in this process on the same box, with HIP events.

    python tools/kv_prefill_bench.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/kv_prefill.json]

Per shape [b, h, h_kv, s, t, d] (fp16, causal: the chunk's s queries are the last s of t tokens), legs on the same values, alternating
over several rounds with every round reported:
 (1) raw     attention_flexible(q, K, V, ..., causal=True, kernel="prefill") on the raw K and V of all t tokens - what an fp16 cache costs;
 (2) packed  attention_flexible_cached(q, cache, causal=True, kernel="prefill") on a cache that holds the t tokens;
 (3) append  the append of the chunk's s tokens at length t - s (a multiple of 16 at every shape: no staging row is read, so the append
             can be repeated at the same length).
`timed` and the buffer rotation are tools/attn_bench.py's: enough distinct q / K / V / caches that the Infinity Cache holds none of
them (the rotation is sized by the packed cache, the smaller of the two).  What is timed is a CALL as a user makes it, Python and
launches included.  Reported per leg: microseconds (median of the rounds) and every round; the bytes of K and V each leg's image pass
reads (fp16, or codes and exponents at 17/16 byte per element); the cache's bytes against the raw K and V; whether the two legs'
outputs are the same bits.  The last shape is a short second turn (16 new tokens over 4096): converting the whole cache is most of
the call - the baseline for a kernel that would read the codes directly.
The criterion: at (1, 32, 32, 512, 4096, 128) and (1, 32, 32, 2048, 8192, 128) the packed leg's MEDIAN is no slower than the SLOWEST
SINGLE ROUND of the raw leg - the main kernel is the same and the image pass reads half the bytes, so the margin is the unchanged
route's own spread - and the outputs of the two legs are the same bits at every shape; `criterion_met` says so per gated shape and the
tool exits non-zero when it does not hold.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
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
from lqer_amd import QuantizedKVCache, attention_flexible, attention_flexible_cached  # noqa: E402

SHAPES = [(1, 32, 32, 512, 4096, 128), (1, 32, 8, 512, 4096, 128), (1, 32, 32, 2048, 8192, 128), (4, 32, 32, 128, 2048, 128),
          (1, 32, 32, 64, 32768, 128), (1, 32, 32, 16, 4096, 128)]
GATED = [(1, 32, 32, 512, 4096, 128), (1, 32, 32, 2048, 8192, 128)]
LEGS = ("raw", "packed", "append")


def one_shape(b, h, hk, s, t, d, cfg, a):
    dt = torch.float16
    past = t - s
    assert past % 16 == 0  # (the cache ends on a block boundary before the chunk: the append reads no staging row and can be repeated)
    cache_bytes = QuantizedKVCache(b, hk, d, cfg, cfg, dt, "cuda", capacity=t).nbytes
    per = b * h * s * d * 2 + cache_bytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // per)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(s + t + d)
    bufs = []
    for _ in range(nbuf):
        q, k, v = (torch.randn(b, hh, n, d, generator=g, device="cuda", dtype=dt) for hh, n in ((h, s), (hk, t), (hk, t)))
        cache = QuantizedKVCache(b, hk, d, cfg, cfg, dt, "cuda", capacity=t)
        cache.append(k[:, :, :past], v[:, :, :past])
        cache.append(k[:, :, past:], v[:, :, past:])
        bufs.append((q, k, v, cache))
    scaling = d ** -0.5

    def append(q, k, v, cache):
        cache.length = past
        cache.append(k[:, :, past:], v[:, :, past:])

    fns = {"raw": lambda q, k, v, cache: attention_flexible(q, k, v, cfg, cfg, scaling, causal=True, out_layout="bshd", kernel="prefill"),
           "packed": lambda q, k, v, cache: attention_flexible_cached(q, cache, scaling, causal=True, out_layout="bshd", kernel="prefill"),
           "append": append}
    same = all(bool(torch.equal(fns["raw"](*buf), fns["packed"](*buf))) for buf in bufs[:2])
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    fns["append"](*bufs[0])
    same = same and bool(torch.equal(fns["raw"](*bufs[0]), fns["packed"](*bufs[0])))  # ... and after the timed appends
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    gated = (b, h, hk, s, t, d) in GATED
    out = {"shape_b_h_hkv_s_t_d": [b, h, hk, s, t, d], "dtype": "float16", "mask": "causal", "buffers": nbuf, "same_bits": same,
           "cache_bytes": cache_bytes, "raw_kv_bytes": 2 * b * hk * t * d * 2, "kv_bytes_read_raw": 2 * b * hk * t * d * 2,
           "kv_bytes_read_packed": 2 * b * hk * t * d * 17 // 16, "gated": gated}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    out["speedup_packed_vs_raw"] = round(med["raw"] / med["packed"], 3)
    out["criterion_met"] = bool(med["packed"] <= max(rounds["raw"])) if gated else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_prefill.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_prefill_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    shapes = []
    with torch.no_grad():
        for sh in SHAPES:
            shapes.append(one_shape(*sh, cfg, a))
            torch.cuda.empty_cache()
    ok = all(s["criterion_met"] for s in shapes if s["gated"]) and all(s["same_bits"] for s in shapes)
    out = {"tool": "tools/kv_prefill_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call included",
           "criterion": "at the gated shapes the packed leg's median no slower than the slowest single round of the raw leg; the two legs' "
                        "outputs the same bits at every shape",
           "criterion_met": ok, "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the packed leg does not meet the criterion at a gated shape (or its output differs from the raw leg's)")


if __name__ == "__main__":
    main()

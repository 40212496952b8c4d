"""Time the decode kernel of the fused quantized attention (lqer_attention_q_decode, csrc/attn_decode.hip) against the two routes a
decode step took before it existed, all in this process on the same box, with HIP events.

    python tools/attn_decode_bench.py [--steps 200] [--warmup 10] [--rounds 5] [--out profiles/attn_decode.json]

Per shape [b, h, h_kv, s, t, d] (fp16, no mask: a decode step sees every key), three legs on the same inputs, alternating over
several rounds with every round reported:
 (1) decode   attention_flexible(..., kernel="decode"): three launches, K and V read once in fp16;
 (2) prefill  attention_flexible(..., kernel="prefill"): lqer_attention_q, two image kernels and the prefill kernel;
 (3) unfused  lqer_eager_attention_forward: the two matmul_flexible products with torch's scale, softmax and cast between them.
`timed` and the buffer rotation are tools/attn_bench.py's (enough distinct q / k / v that the Infinity Cache does not hold them).
What is timed is a CALL as a user of attention_flexible makes it, Python and launches included: below about t = 4096 at batch 1 that
host side (45 us for either fused kernel, 90 us for the unfused chain of torch ops) is longer than the kernels, so those rows compare
what a call costs, not kernels, and their GB/s are not kernel rates; device-only times are not measured here.  Reported per leg: microseconds (median of the rounds), effective GB/s on the model "K and V once in fp16,
plus q, plus out, plus the workspace traffic of the decode kernel" (S2, the chunk statistics and the partial outputs counted as
written once and read once - an approximation: pass 2 reads a row's chunk statistics again in every chunk's workgroup, mostly from
L2 - the same byte count for all three legs, so the GB/s compare), and that as a fraction of the HBM peak.
The speed criterion: at every shape the automatic rule sends to the decode kernel, the decode leg's MEDIAN must be below the FASTEST
SINGLE ROUND of both other legs; `criterion_met` says so per shape, `auto_kernel` what the rule picks, `routing_ok` whether the rule
agrees with the measurement (a shape the decode kernel loses must go to the leg that won), and the tool exits non-zero when it does
not.  PROBES are further shapes, timed the same way, that place the rule's thresholds; they are reported under `probes` and gated
the same way.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attn_bench import L3_BYTES, timed  # noqa: E402
from benchlib.workloads import HBM_PEAK_GBS  # noqa: E402
from lqer_amd import attention as A  # noqa: E402
from lqer_amd import attention_flexible  # noqa: E402

SHAPES = [  # b, h, h_kv, s, t, d
    (1, 32, 32, 1, 2048, 128), (8, 32, 32, 1, 2048, 128), (1, 32, 8, 1, 4096, 128), (1, 32, 32, 4, 2048, 128), (1, 32, 32, 8, 2048, 128),
    (1, 32, 32, 1, 128, 128), (1, 32, 32, 1, 32768, 128),
]
PROBES = [  # where the automatic rule's thresholds sit: batch x kv_heads between 32 and 256, short and long t at batch 8, short t at batch 1
    (2, 32, 32, 1, 2048, 128), (4, 32, 32, 1, 2048, 128), (8, 32, 32, 1, 128, 128), (8, 32, 32, 1, 512, 128), (8, 32, 32, 1, 8192, 128),
    (1, 32, 32, 1, 512, 128), (1, 32, 32, 1, 8192, 128), (8, 32, 8, 1, 2048, 128),
]
LEGS = ("decode", "prefill", "unfused")


def model_bytes(b, h, hk, s, t, d):
    """K and V once in fp16 + q + out + the decode kernel's workspace traffic (include/lqer_hip.h: chunks of
    C = 16 min(max(ceil(t / 256), 1), 8) keys; S2, chunk statistics and partial outputs in fp32, each counted as written once and read
    once - pass 2 in fact reads a row's nch statistics in each of its nch workgroups, small and mostly from L2: an approximation)."""
    c = 16 * min(max(-(-t // 256), 1), 8)
    nch, rows = -(-t // c), b * h * s
    ws = rows * nch * c * 4 + rows * nch * 2 * 4 + rows * nch * d * 4
    return 2 * b * hk * t * d * 2 + 2 * b * h * s * d * 2 + 2 * ws


def one_shape(b, h, hk, s, t, d, cfg, a):
    dt = torch.float16
    per = (b * h * s * d + 2 * b * hk * t * d) * 2
    nbuf = max(3, min(64, -(-3 * L3_BYTES // per)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(s + t + d)
    bufs = [(torch.randn(b, h, s, d, generator=g, device="cuda", dtype=dt), torch.randn(b, hk, t, d, generator=g, device="cuda", dtype=dt),
             torch.randn(b, hk, t, d, generator=g, device="cuda", dtype=dt)) for _ in range(nbuf)]
    scaling = d ** -0.5
    mod = types.SimpleNamespace(_lqer_matmul_cfg=(cfg, cfg), num_key_value_groups=h // hk, training=False)
    fns = {
        "decode": lambda q, k, v: attention_flexible(q, k, v, cfg, cfg, scaling, out_layout="bshd", kernel="decode"),
        "prefill": lambda q, k, v: attention_flexible(q, k, v, cfg, cfg, scaling, out_layout="bshd", kernel="prefill"),
        "unfused": lambda q, k, v: A.lqer_eager_attention_forward(mod, q, k, v, None, scaling)[0],
    }
    auto = attention_flexible.kernel(*bufs[0], cfg, cfg)
    outs = {leg: fns[leg](*bufs[0]).float() for leg in LEGS}
    rel = {leg: float((outs["decode"] - outs[leg]).norm() / outs[leg].norm()) for leg in ("prefill", "unfused")}
    del outs
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    nbytes = model_bytes(b, h, hk, s, t, d)
    gbs = lambda us: nbytes / (us * 1e-6) / 1e9
    met = bool(med["decode"] < min(rounds["prefill"]) and med["decode"] < min(rounds["unfused"]))
    out = {"shape_b_h_hkv_s_t_d": [b, h, hk, s, t, d], "dtype": "float16", "buffers": nbuf, "model_bytes": nbytes, "auto_kernel": auto,
           "criterion_met": met,
           "fastest_leg": min(LEGS, key=lambda leg: med[leg]),
           "rel_l2_decode_vs_prefill": float(f"{rel['prefill']:.3e}"), "rel_l2_decode_vs_unfused": float(f"{rel['unfused']:.3e}")}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
        out[f"gb_s_{leg}"] = round(gbs(med[leg]), 1)
        out[f"frac_of_hbm_peak_{leg}"] = round(gbs(med[leg]) / HBM_PEAK_GBS, 4)
    out["speedup_vs_prefill"] = round(med["prefill"] / med["decode"], 2)
    out["speedup_vs_unfused"] = round(med["unfused"] / med["decode"], 2)
    # what the automatic rule does with this shape, and whether that agrees with the measurement: the decode kernel where it meets the
    # criterion, else the leg with the smaller median
    won = "decode" if met else min(("prefill", "unfused"), key=lambda leg: med[leg])
    out["routing_ok"] = bool((auto or "unfused") == won)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    with torch.no_grad():
        shapes = [one_shape(*sh, cfg, a) for sh in SHAPES]
        probes = [one_shape(*sh, cfg, a) for sh in PROBES]
    out = {"tool": "tools/attn_decode_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "steps": a.steps, "rounds": a.rounds, "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call included",
           "criterion": "decode median below the fastest single round of the prefill leg and of the unfused leg, at every shape the automatic rule "
                        "sends to the decode kernel",
           "all_routed_shapes_meet_criterion": all(s["routing_ok"] for s in shapes + probes), "shapes": shapes, "probes": probes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not out["all_routed_shapes_meet_criterion"]:
        raise SystemExit("the automatic rule does not follow the measurement at some shape (routing_ok false)")


if __name__ == "__main__":
    main()

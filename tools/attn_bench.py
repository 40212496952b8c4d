"""Time the fused quantized attention against the unfused route it replaces, both in this process on the same box, with HIP events.

    python tools/attn_bench.py [--steps 10] [--warmup 3] [--rounds 3] [--out profiles/attn_fused.json]

Per shape [b, h, s, t, d] (fp16):
 (a) one `attention_flexible` call (lqer_attention_q, csrc/attn_q.hip: two image kernels and the attention kernel), output [b, s, h, d];
 (b) the body of `lqer_eager_attention_forward` as it stands (matmul_flexible, scale, mask add, fp32 softmax, cast, matmul_flexible,
     transpose copy) on the same inputs,
alternating the two over several rounds (every round is reported, the derived figures use the medians), rotating over enough distinct q / k / v buffers that the 256 MiB
Infinity Cache does not hold them.  Shapes: Llama-7B prefill [1, 32, 2048, 2048, 128] with the [1, 1, s, t] mask tensor and with
causal = 1, [4, 32, 512, 512, 128], an OPT-like d = 64, and one decode step (s = 1, t = 2048).  Reported per leg: microseconds,
algorithmic TFLOP/s on 4 b h s t d (half of it under the causal rule), that as a fraction of the bf16 MFMA peak, and the unfused
chain's effective GB/s on a traffic model of twelve passes over the [b h, s, t] scores (the fp32 softmax result counts twice).
Not part of bench.py.  Prints one JSON line and writes it.  Needs a GPU: there is no fall-back."""
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

from benchlib.workloads import HBM_PEAK_GBS  # noqa: E402
from lqer_amd import attention as A  # noqa: E402
from lqer_amd import attention_flexible  # noqa: E402

L3_BYTES = 256 << 20
BF16_PEAK_TFLOPS = 2500.0
GATES = {"llama7b_prefill_mask": 1.5, "llama7b_prefill_causal": 2.0}  # fused at least this much faster than the unfused route
SHAPES = [  # name, b, h, h_kv, s, t, d, mask form
    ("llama7b_prefill_mask", 1, 32, 32, 2048, 2048, 128, "mask"),
    ("llama7b_prefill_causal", 1, 32, 32, 2048, 2048, 128, "causal"),
    ("batch4_s512_causal", 4, 32, 32, 512, 512, 128, "causal"),
    ("opt_like_d64_mask", 1, 32, 32, 2048, 2048, 64, "mask"),
    ("decode_s1_t2048", 1, 32, 32, 1, 2048, 128, "none"),
]


def timed(fn, bufs, steps, warmup):
    for i in range(warmup):
        fn(*bufs[i % len(bufs)])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(steps):
        fn(*bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3  # us


def one_shape(name, b, h, hk, s, t, d, form, cfg, a):
    dt = torch.float16
    per = (b * h * s * d + 2 * b * hk * t * d) * 2
    nbuf = max(3, min(64, -(-3 * L3_BYTES // per)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(s + t + d)
    bufs = [(torch.randn(b, h, s, d, generator=g, device="cuda", dtype=dt), torch.randn(b, hk, t, d, generator=g, device="cuda", dtype=dt),
             torch.randn(b, hk, t, d, generator=g, device="cuda", dtype=dt)) for _ in range(nbuf)]
    scaling = d ** -0.5
    i, j = torch.arange(s, device="cuda")[:, None], torch.arange(t, device="cuda")[None, :]
    mask = None if form == "none" else torch.zeros(1, 1, s, t, device="cuda", dtype=dt).masked_fill_(j > i + (t - s), torch.finfo(dt).min)
    mod = types.SimpleNamespace(_lqer_matmul_cfg=(cfg, cfg), num_key_value_groups=h // hk, training=False)

    def fused(q, k, v):
        return attention_flexible(q, k, v, cfg, cfg, scaling, attention_mask=mask if form == "mask" else None, causal=form == "causal", out_layout="bshd")

    def unfused(q, k, v):
        return A.lqer_eager_attention_forward(mod, q, k, v, mask, scaling)[0]

    assert attention_flexible.route(*bufs[0], cfg, cfg, mask if form == "mask" else None, form == "causal") == "fused"
    got, want = fused(*bufs[0]), unfused(*bufs[0])
    rel = float((got.float() - want.float()).norm() / want.float().norm())
    rounds = {"fused": [], "unfused": []}
    for _ in range(a.rounds):
        rounds["fused"].append(timed(fused, bufs, a.steps, a.warmup))
        rounds["unfused"].append(timed(unfused, bufs, a.steps, a.warmup))
    res = {k: statistics.median(v) for k, v in rounds.items()}  # every round is reported; the figures below are on the medians
    flop = 4.0 * b * h * s * t * d * (0.5 if form == "causal" else 1.0)
    score_bytes = b * h * s * t * 2
    tf = lambda us: flop / (us * 1e-6) / 1e12
    out = {"name": name, "shape_b_h_s_t_d": [b, h, s, t, d], "kv_heads": hk, "dtype": "float16", "mask": form, "buffers": nbuf,
           "us_fused": round(res["fused"], 1), "us_unfused": round(res["unfused"], 1),
           "us_fused_rounds": [round(x, 1) for x in rounds["fused"]], "us_unfused_rounds": [round(x, 1) for x in rounds["unfused"]],
           "speedup_rounds": [round(u / f, 3) for f, u in zip(rounds["fused"], rounds["unfused"])], "speedup": round(res["unfused"] / res["fused"], 3),
           "algorithmic_gflop": round(flop / 1e9, 2), "tflops_fused": round(tf(res["fused"]), 1), "tflops_unfused": round(tf(res["unfused"]), 1),
           "fused_frac_of_bf16_peak": round(tf(res["fused"]) / BF16_PEAK_TFLOPS, 4),
           "unfused_frac_of_bf16_peak": round(tf(res["unfused"]) / BF16_PEAK_TFLOPS, 4),
           "unfused_model_bytes_12_passes": 12 * score_bytes, "unfused_effective_gb_s": round(12 * score_bytes / (res["unfused"] * 1e-6) / 1e9, 1),
           "rel_l2_fused_vs_unfused": float(f"{rel:.3e}")}
    if name in GATES:
        out["gate_speedup"] = GATES[name]
        out["gate_met"] = bool(res["unfused"] / res["fused"] >= GATES[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_fused.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    with torch.no_grad():
        shapes = [one_shape(*sh, cfg, a) for sh in SHAPES]
    out = {"tool": "tools/attn_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "bf16_peak_tflops": BF16_PEAK_TFLOPS, "steps": a.steps, "rounds": a.rounds, "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

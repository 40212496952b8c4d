"""Time the calibration kernel against the reference's hook body, both in this process on the same box, with HIP events.

    python tools/calib_bench.py [--steps 20] [--warmup 5] [--rounds 3]

Per dtype (fp16, fp32) and shape (8192 x 4096, 8192 x 11008: batch_size 4 x max_length 2048 at Llama-7B's two K):
 (a) one `ops.col_abs_stats` call updating a running scale (csrc/col_stats.hip),
 (b) the reference's hook body written out in torch (statistic_profiler/scale.py:32-38):
     torch.maximum(scale, x.float().abs().view(-1, K).mean(0)),
alternating the two over several rounds (the last round is kept), rotating over enough distinct input buffers that the 256 MiB
Infinity Cache does not hold them.  Then the end-to-end time of `profile_model` over a Llama-7B-shaped stack of hooked Linears
(one decoder layer's seven projections, fp16, 8192 tokens) with and without the hooks.  Not part of bench.py.  Prints one JSON line
and writes it to profiles/calib_col_stats.json.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.workloads import HBM_PEAK_GBS  # noqa: E402
from lqer_amd import calibrate, ops  # noqa: E402

L3_BYTES = 256 << 20


def timed(fn, bufs, steps, warmup):
    for i in range(warmup):
        fn(bufs[i % len(bufs)])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(steps):
        fn(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def one_shape(M, K, dt, a):
    es = 2 if dt == torch.float16 else 4
    nbuf = max(3, -(-3 * L3_BYTES // (M * K * es)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(K)
    bufs = [torch.randn(4, M // 4, K, generator=g, device="cuda", dtype=dt) for _ in range(nbuf)]
    run_k, run_t = torch.zeros(K, device="cuda"), [torch.zeros(K, device="cuda")]

    def kernel(x):
        ops.col_abs_stats(x, run=run_k)

    def hook_body(x):
        xf = x.float()
        run_t[0] = torch.maximum(run_t[0], xf.abs().view(-1, x.shape[-1]).mean(0))

    res = {}
    for _ in range(a.rounds):
        res["kernel"] = timed(kernel, bufs, a.steps, a.warmup)
        res["torch"] = timed(hook_body, bufs, a.steps, a.warmup)
    elems = M * K
    by_k = elems * es + 2 * 2 * 4 * min(64, -(-M // 64)) * K  # x once + the partials written and read (an upper bound on their count)
    by_t = elems * (18 if es == 2 else 12)                    # fp32 copy (fp16 only), abs copy, column mean
    gbs = by_k / (res["kernel"] * 1e-3) / 1e9
    return {"M": M, "K": K, "dtype": str(dt).split(".")[-1], "buffers": nbuf, "ms_kernel": round(res["kernel"], 4),
            "ms_torch_hook_body": round(res["torch"], 4), "ratio": round(res["torch"] / res["kernel"], 2),
            "bytes_kernel": by_k, "bytes_torch_hook_body": by_t, "traffic_ratio": round(by_t / by_k, 2),
            "kernel_gb_s": round(gbs, 1), "kernel_frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
            "torch_gb_s": round(by_t / (res["torch"] * 1e-3) / 1e9, 1)}


class Stack(torch.nn.Module):
    """one Llama-7B decoder layer's seven projections, each fed a tensor of its input width"""

    def __init__(self):
        super().__init__()
        shapes = [(4096, 4096)] * 4 + [(4096, 11008)] * 2 + [(11008, 4096)]
        self.proj = torch.nn.ModuleList([torch.nn.Linear(k, n, bias=False) for k, n in shapes])

    def forward(self, x4096, x11008):
        for p in self.proj:
            p(x4096 if p.in_features == 4096 else x11008)


def end_to_end(a):
    model = Stack().half().cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    batches = [(torch.randn(4, 2048, 4096, generator=g, device="cuda", dtype=torch.float16),
                torch.randn(4, 2048, 11008, generator=g, device="cuda", dtype=torch.float16)) for _ in range(4)]

    def run(hooks):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if hooks:
            calibrate.profile_model(model, batches)
        else:
            with torch.no_grad():
                for b in batches:
                    model(*b)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(batches)

    out = {}
    for _ in range(a.rounds):
        out["ms_per_batch_without_hooks"] = round(run(False), 3)
        out["ms_per_batch_profile_model"] = round(run(True), 3)
    out["overhead"] = round(out["ms_per_batch_profile_model"] / out["ms_per_batch_without_hooks"] - 1, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calib_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    shapes = [one_shape(8192, K, dt, a) for dt in (torch.float16, torch.float32) for K in (4096, 11008)]
    out = {"tool": "tools/calib_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "accept": {"float16": 4.5, "float32": 1.5, "at_K": 11008}, "shapes": shapes, "profile_model_llama7b_layer_fp16": end_to_end(a)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "calib_col_stats.json"), "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

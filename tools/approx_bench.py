"""Time lqer_factors' two methods against each other, in this process on the same box, with HIP events.

    python tools/approx_bench.py [--steps 5] [--warmup 2] [--out profiles/approx_subspace.json]

Per shape (N x K, rank: 4096 x 4096 r = 32, 11008 x 4096 r = 32, 4096 x 11008 r = 32, 4096 x 4096 r = 128; fp16 W, MXINT4 weight blocks
of 16, fp32 factors) and with / without an activation scale:
 (a) method="svd": quantize, materialise E^T in fp32, torch.linalg.svd (full) - the only route before method="subspace" existed; ONE timed
     call per entry behind a small warm-up decomposition (a full SVD takes seconds: the spread of one call is far below the difference),
 (b) method="subspace" (oversample 16, power_iters 2): `steps` timed calls behind `warmup`,
 (c) the 2 + 2 power_iters products of (b) alone - ops.qerr_matmul on fixed operands - and their rate over W's bytes (one read of W per
     product: the kernel's traffic model; the partials in the workspace come on top),
 (d) peak extra device memory of (a) and (b) (torch's allocator, W itself excluded),
 (e) the reconstruction error |E_s - U_r diag(sigma_r) V_r^T| / |E_s| before the A / B quantizers: the SVD's (the optimum) and the
     subspace iteration's at power_iters 1, 2 and 4.
Not part of bench.py.  Prints one JSON line per entry, and writes the whole result after every entry.  Needs a GPU: no fall-back."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.workloads import HBM_PEAK_GBS  # noqa: E402
from lqer_amd import approximate, ops  # noqa: E402

W_CFG = dict(name="block_fp", width=4, exponent_width=8, exponent_bias=None, block_size=[1, 16], skip_first_dim=False)
SHAPES = [(4096, 4096, 32), (4096, 4096, 128), (11008, 4096, 32), (4096, 11008, 32)]
OVERSAMPLE, POWER_ITERS = 16, 2


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base, e0.elapsed_time(e1)


def one_entry(N, K, r, with_scale, a):
    g = torch.Generator(device="cuda").manual_seed(N + K + r)
    W = (0.02 * torch.randn(N, K, generator=g, device="cuda")).half()
    W[:, 5] *= 20
    s = (0.5 + torch.rand(K, generator=g, device="cuda")) if with_scale else None
    l = min(r + OVERSAMPLE, N, K)

    svd = lambda: approximate.lqer_factors(W, W_CFG, r, None, None, s)  # noqa: E731
    sub = lambda: approximate.lqer_factors(W, W_CFG, r, None, None, s, method="subspace")  # noqa: E731
    (A_svd, B_svd), mem_svd, ms_svd = peak_extra(svd)  # (the one timed call: seconds, against microseconds of first-launch costs)
    _, mem_sub, _ = peak_extra(sub)
    ms_sub = timed(sub, a.steps, a.warmup)

    X1 = torch.randn(N, l, generator=g, device="cuda")
    X0 = torch.randn(K, l, generator=g, device="cuda")
    ms_t1 = timed(lambda: ops.qerr_matmul(W, W_CFG, X1, 1, s), 4 * a.steps, a.warmup)
    ms_t0 = timed(lambda: ops.qerr_matmul(W, W_CFG, X0, 0, s), 4 * a.steps, a.warmup)
    n_prod = 2 + 2 * POWER_ITERS
    ms_products = (1 + POWER_ITERS) * ms_t1 + (1 + POWER_ITERS) * ms_t0
    w_bytes = N * K * 2

    Wf = W.float()
    Es = (Wf - ops.quantize_mxint(Wf, ops.make_qfmt(W_CFG, "w"), want=("deq",))["deq"]).t()
    if s is not None:
        Es = s[:, None] * Es
    nrm = float(Es.norm())
    US = A_svd if s is None else s[:, None] * A_svd
    err = {"svd": float((Es - US @ B_svd).norm()) / nrm}
    for p in (1, 2, 4):
        U, B = approximate._subspace_factors(W, W_CFG, r, s, OVERSAMPLE, p, 0)
        err[f"subspace_power_iters_{p}"] = float((Es - U @ B).norm()) / nrm
    return {"N": N, "K": K, "rank": r, "columns": l, "scale": with_scale, "ms_svd": round(ms_svd, 2), "svd_timed_calls": 1,
            "ms_subspace": round(ms_sub, 3), "svd_over_subspace": round(ms_svd / ms_sub, 1),
            "ms_qerr_matmul_trans0": round(ms_t0, 4), "ms_qerr_matmul_trans1": round(ms_t1, 4), "products": n_prod,
            "ms_in_qerr_matmul": round(ms_products, 3), "qerr_share_of_subspace": round(ms_products / ms_sub, 3),
            "gb_s_over_w_trans0": round(w_bytes / (ms_t0 * 1e-3) / 1e9, 1), "gb_s_over_w_trans1": round(w_bytes / (ms_t1 * 1e-3) / 1e9, 1),
            "frac_of_hbm_peak_trans0": round(w_bytes / (ms_t0 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "frac_of_hbm_peak_trans1": round(w_bytes / (ms_t1 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "peak_extra_bytes_svd": mem_svd, "peak_extra_bytes_subspace": mem_sub, "reconstruction_error": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_subspace.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("approx_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    torch.linalg.svd(torch.randn(512, 512, device="cuda"), full_matrices=False)  # (loads the solver library)
    out = {"tool": "tools/approx_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "w": "fp16, MXINT4 blocks of 16", "oversample": OVERSAMPLE, "power_iters": POWER_ITERS, "steps": a.steps, "entries": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for N, K, r in SHAPES:
        for with_scale in (False, True):
            out["entries"].append(one_entry(N, K, r, with_scale, a))
            print(json.dumps(out["entries"][-1]), flush=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Time a Linear forward with the compact image of a 2- / 3-bit weight (weight_image = "narrow") against the standard 4.5-bit image of
the very same module weights, in one process, with HIP events (benchlib.hipevents) - the yardstick is this build's standard route.

    python tools/narrow_weight_bench.py [--rounds 20] [--rotate 48] [--out profiles/narrow_weights.json]

Formats: W2 in blocks of 16 under A8-MXINT (bench.MXINT_Q with a 2-bit w_quantizer, rank 32) and bench.W3A16_Q (fp16, rank 64).
Shapes: the three Llama-7B projections (4096 x 4096, 4096 -> 11008, 11008 -> 4096) at M = 1, 8, 64 - where the decode-size kernels
read the compact image directly - and at M = 2048, where the forward widens it into the workspace and runs the tile kernel.
Every leg walks `rotate` distinct copies of its weight image round robin (48 x 9.4 MB and more: nothing is re-read from the 256 MB
Infinity Cache - benchlib.runner's rotation for the single-Linear decode workloads), through the C ABI as the module calls it; one
round = one event pair around `rotate` calls, a row = the median over the rounds and their spread (min, max).  Per row: the bytes of
both images, narrow / standard as a time ratio beside the byte ratio, whether the outputs are the same bits, which route
lqer_weight_narrow_route names, and at M = 2048 the widen kernel's own time.  `slower_beyond_spread` marks a decode row whose narrow
median lies above the standard leg's slowest round.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.hipevents import HipEvent  # noqa: E402
from benchlib.workloads import MXINT_Q, W3A16_Q, _bfp, make_case  # noqa: E402

SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096)]  # (K, N)
TOKENS = [1, 8, 64, 2048]
FORMATS = {"W2b16-A8MXINT": (dict(MXINT_Q, w_quantizer=_bfp(2, [1, 16], False)), 32, True),
           "W3b32-A16": (W3A16_Q, 64, False)}  # name -> (q_config, rank, A / B snapped to 8-bit MXINT)
EV_FLAGS = 0x20000000  # hipEventDisableSystemFence (benchlib.hipevents)


def _stats(us):
    return {"median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3)}


def _timed(calls, stream, rounds, warmup=2):
    """calls: one closure per rotated image; per-call microseconds of every round."""
    e0, e1 = HipEvent(EV_FLAGS), HipEvent(EV_FLAGS)
    out = []
    for r in range(warmup + rounds):
        e0.record(stream)
        for c in calls:
            c()
        e1.record(stream)
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3 / len(calls))
    return out


def one_format(name, cfg, rank, quantize_ab, K, N, a, rows):
    import lqer_amd
    from lqer_amd import _lib, ops

    L = _lib.lib()
    dev = "cuda:0"
    x, W, A, B = make_case(max(TOKENS), K, N, rank, seed=11, quantize_ab=quantize_ab)
    mods = {}
    for kind in ("standard", "narrow"):
        m = lqer_amd.LinearFlexibleLqer(K, N, bias=False, q_config=cfg, l_config={"rank": rank})
        m.load_state_dict({"weight": W, "A": A, "B": B})
        m.weight_image = kind
        m = m.to(dev).half()
        m.pack()
        m.weight.data = torch.empty(0, device=dev, dtype=torch.float16)  # (the images are what the calls read)
        mods[kind] = m
    xd_all = x.half().to(dev)
    st = ops._stream(torch.device(dev))
    imgs = {k: [m._packed["w"]] + [m._packed["w"].clone() for _ in range(a.rotate - 1)] for k, m in mods.items()}
    fmt = mods["narrow"]._fmt["w"]
    nbytes = {k: int(v[0].numel()) for k, v in imgs.items()}
    assert nbytes["narrow"] == ops.weight_narrow_bytes(N, K, fmt)
    for M in TOKENS:
        xd = xd_all[:M].contiguous()
        legs, ys = {}, {}
        for kind, m in mods.items():
            desc = m._desc()
            dt = ops.dtype_code(xd)
            narrow = kind == "narrow"
            ws_bytes = L.lqer_linear_forward_narrow_workspace_bytes(C.byref(desc), M) if narrow else ops.linear_sizes(desc, M).workspace
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            a_t, a_limbs = m._side_image(M, desc, dt)
            p = m._packed
            y = torch.empty(M, N, dtype=torch.float16, device=dev)
            fwd = L.lqer_linear_forward_narrow if narrow else L.lqer_linear_forward
            rest = (a_t, ops._ptr(p.get("b_t")), a_limbs, p.get("b_limbs", 0), ops._ptr(p.get("bias")), y.data_ptr(), N, ws.data_ptr(), ws_bytes, st)

            def call(w, fwd=fwd, desc=desc, xd=xd, dt=dt, M=M, rest=rest):
                rc = fwd(C.byref(desc), xd.data_ptr(), dt, M, K, w.data_ptr(), *rest)
                if rc:
                    _lib.check(rc, "forward")

            call(imgs[kind][0])
            torch.cuda.synchronize()
            ys[kind] = y.clone()
            legs[kind] = _timed([(lambda w=w: call(w)) for w in imgs[kind]], st, a.rounds)
            if narrow:
                route = L.lqer_weight_narrow_route(C.byref(desc), M, dt, K, int(p.get("a_limbs", 0)), int(p.get("b_limbs", 0)))
        s_std, s_nar = _stats(legs["standard"]), _stats(legs["narrow"])
        row = {"format": name, "K": K, "N": N, "M": M, "rank": rank,
               "route": {1: "direct", 2: "direct, one launch", 3: "widen"}.get(route, str(route)),
               "image_bytes": nbytes, "byte_ratio": round(nbytes["narrow"] / nbytes["standard"], 4),
               "standard": s_std, "narrow": s_nar, "time_ratio": round(s_nar["median_us"] / s_std["median_us"], 4),
               "same_bits": bool(torch.equal(ys["standard"], ys["narrow"]))}
        if M <= 64:
            row["slower_beyond_spread"] = bool(s_nar["median_us"] > s_std["max_us"])
        else:
            wide = torch.empty(nbytes["standard"], dtype=torch.uint8, device=dev)
            row["widen_kernel"] = _stats(_timed([(lambda w=w: _lib.check(L.lqer_weight_widen(w.data_ptr(), N, K, C.byref(fmt), wide.data_ptr(), st), "widen"))
                                                 for w in imgs["narrow"]], st, a.rounds))
        rows.append(row)
        print(json.dumps(row), flush=True)
    del imgs, mods
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rotate", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrow_weights.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for K, N in SHAPES:
        for name, (cfg, rank, qab) in FORMATS.items():
            one_format(name, cfg, rank, qab, K, N, a, rows)
    doc = {"tool": "tools/narrow_weight_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "rotate": a.rotate,
           "note": "per-call microseconds: one HIP event pair around `rotate` calls, each on another copy of the weight image; "
                   "median / min / max over the rounds; standard and narrow legs on the same module weights in one process",
           "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r for r in rows if r.get("slower_beyond_spread") or not r["same_bits"]]
    print(f"wrote {a.out}: {len(rows)} rows, {len(bad)} decode rows slower than the standard leg's slowest round or with other bits")


if __name__ == "__main__":
    main()

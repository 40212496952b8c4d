"""Time the minifloat Linear forward against the MXINT one at the C2 shape (M 2048, 4096 x 4096, rank 32), both in this process,
with HIP events around back-to-back module forwards (fp16 tensors, as bench.py's C2).

    python tools/minifloat_time.py [--steps 50] [--warmup 10]

minifloat: W minifloat(4, 2, 7); x, b and - by the reference's fall-back - A_out / B_out minifloat(8, 4, 7).  Not part of bench.py.
Prints one JSON line: ms per forward of each and their ratio."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lqer_amd  # noqa: E402
from benchlib.workloads import MXINT_Q, make_case  # noqa: E402

MF8 = dict(name="minifloat", width=8, exponent_width=4, exponent_bias=7)
MF_Q = dict(name="flexible_lqer", is_ptq=True, default=False, x_quantizer=MF8, b_quantizer=MF8,
            w_quantizer=dict(name="minifloat", width=4, exponent_width=2, exponent_bias=7))


def timed(mod, x, steps, warmup):
    for _ in range(warmup):
        mod(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        mod(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    M, K, N, r = 2048, 4096, 4096, 32
    x, W, A, B = make_case(M, K, N, r, seed=7)
    xd = x.half().cuda()
    mods = {}
    for name, qc in (("mxint", MXINT_Q), ("minifloat", MF_Q)):
        m = lqer_amd.LinearFlexibleLqer(K, N, bias=False, q_config=qc, l_config={"rank": r})
        m.load_state_dict({"weight": W, "A": A, "B": B})
        mods[name] = m.cuda().half()
    res = {}
    for rnd in range(2):  # interleaved rounds: the second is kept (clocks settled)
        for name, m in mods.items():
            res[name] = timed(m, xd, a.steps, a.warmup)
    out = {"shape": [M, K, N, r], "ms_mxint": round(res["mxint"], 4), "ms_minifloat": round(res["minifloat"], 4),
           "ratio": round(res["minifloat"] / res["mxint"], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

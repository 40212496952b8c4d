#!/usr/bin/env python3
"""A/B timing of the STANDALONE quantizer kernels (quantize.hip) across library builds, interleaved rounds in one process:
lqer_quantize_act_mxint (the bf16 activation image) and lqer_quantize_mxint (dequantized fp32 values) per caller dtype, over
  seg16   block_fp, blocks of 16          -> k_quant_seg16<DT, VEC>   (image and values; aligned rows and rows whose stride is not)
  blk32   block_fp, blocks of 32          -> k_quant_blk<DT>
  row     block_fp, one exponent per row  -> k_quant_row<DT>
  int     integer (fixed point)           -> k_quant_int<DT>
  mf      minifloat e4m3                  -> k_quant_mf<DT, VEC>      (aligned / not)
usage: python tools/ab_quantize.py [--rows 2048 --cols 4096 --rounds 8 --iters 20] [--json FILE] lib_a.so lib_b.so ...
Every build's output is compared with the first build's (same bits or the tool fails)."""
import argparse, ctypes as C, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lqer_amd import _lib
from tools.ab_gemm import load

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2048); ap.add_argument("--cols", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=8); ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--json", default=None)
ap.add_argument("libs", nargs="+")
args = ap.parse_args()
R, K = args.rows, args.cols
dev = torch.device("cuda:0")
libs = [(os.path.basename(p), load(p)) for p in args.libs]
FMT = {"seg16": _lib.QFmt(_lib.Q_MXINT, 8, 16, 8, 127), "blk32": _lib.QFmt(_lib.Q_MXINT, 8, 32, 8, 127), "row": _lib.QFmt(_lib.Q_MXINT, 8, -1, 8, 127),
       "int": _lib.QFmt(_lib.Q_INT, 8, -1, 1, 4), "mf": _lib.QFmt(_lib.Q_MINIFLOAT, 8, -1, 4, 7)}
DT = {"f32": (torch.float32, _lib.F32), "f16": (torch.float16, _lib.F16), "bf16": (torch.bfloat16, _lib.BF16)}
# (case, format, entry point, row stride): stride K = 16-byte aligned rows, K + 2 = not (8 bytes off for fp32, 4 for the 16-bit types)
CASES = [("seg16_image", "seg16", "act", K), ("seg16_image_unaligned", "seg16", "act", K + 2), ("seg16_values", "seg16", "deq", K),
         ("blk32_values", "blk32", "deq", K), ("row_values", "row", "deq", K), ("row_image", "row", "act", K), ("int_values", "int", "deq", K),
         ("mf_values", "mf", "deq", K), ("mf_values_unaligned", "mf", "deq", K + 2)]
Mp, Kp = libs[0][1].lqer_padded_m(R), libs[0][1].lqer_padded_k(K)
result = {}
for case, fk, entry, ld in CASES:
    for dn, (tdt, code) in DT.items():
        torch.manual_seed(1)
        buf = torch.randn(R, ld, device=dev).to(tdt)
        x = buf[:, :K]
        out = torch.zeros(Mp * Kp, dtype=torch.bfloat16, device=dev) if entry == "act" else torch.zeros(R * K, dtype=torch.float32, device=dev)
        fmt = FMT[fk]
        def call(L):
            if entry == "act":
                return L.lqer_quantize_act_mxint(x.data_ptr(), code, R, K, ld, C.byref(fmt), out.data_ptr(), None)
            return L.lqer_quantize_mxint(x.data_ptr(), code, R, K, ld, C.byref(fmt), out.data_ptr(), None, None, None)
        res = {n: [] for n, _ in libs}
        ref = None
        for rnd in range(args.rounds):
            for n, L in libs:
                for _ in range(3):
                    rc = call(L)
                    assert rc == 0, (case, dn, n, L.lqer_last_error())
                torch.cuda.synchronize()
                if rnd == 0:
                    got = out.clone()
                    ref = got if ref is None else ref
                    assert torch.equal(got.view(torch.int16 if entry == "act" else torch.int32), ref.view(torch.int16 if entry == "act" else torch.int32)), (case, dn, n, "output differs from " + libs[0][0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    call(L)
                e1.record(); torch.cuda.synchronize()
                res[n].append(e0.elapsed_time(e1) / args.iters * 1e3)
        row = {}
        for n, v in res.items():
            s = sorted(v)
            row[n] = {"median_us": round(s[len(s) // 2], 3), "min_us": round(s[0], 3), "rounds_us": [round(t, 3) for t in v]}
        result[f"{case}_{dn}"] = row
        print(f"{case:24s} {dn:4s} " + "  ".join(f"{n} median {r['median_us']:8.2f} min {r['min_us']:8.2f}" for n, r in row.items()) + "  us (same bits)")
if args.json:
    json.dump({"rows": R, "cols": K, "rounds": args.rounds, "iters": args.iters, "cases": result}, open(args.json, "w"), indent=1)

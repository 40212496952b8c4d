"""Time the step between the up / gate projections and the down projection of a Llama-7B MLP layer, two ways, in one process:

    leg A   h = F.silu(g) * u as two torch launches, then down_proj(h)         (the module's forward: lqer_linear_forward)
    leg B   down_proj.forward_gated(g, u)                                      (lqer_linear_forward_gated: csrc/act_gated.hip + the GEMM)

    python tools/gated_mlp_bench.py [--rounds 20] [--rotate 12] [--out profiles/gated_mlp.json]

Shape: the down projection K = 11008 -> N = 4096, rank 32, W4A8 MXINT in blocks of 16 (bench.MXINT_Q), fp16, at M = 1, 8, 64, 2048.
Method: every call of a round works on another of `rotate` copies of (g, u) AND of the module - 12 x (25 MB weight image + up to 90 MB
of g and u) - so no operand is served from the 256 MB Infinity Cache; 2 warm-up rounds; a round = one HIP event pair (benchlib.hipevents)
around `rotate` calls of one leg, the legs alternating round by round; a row = the median over the rounds with their spread (min, max).
What is timed is a CALL as a user makes it, Python and ctypes included, on both legs alike.  Per leg also the launches (by construction:
two torch kernels + the forward's - one at M <= 8, two above; the fused leg: two) and the algorithmic bytes computed from the shapes.
`slower_beyond_spread` marks a size where leg B's median lies above leg A's slowest round.  `act_kernel` is lqer_quantize_act_xa_gated
alone through the C ABI on the same rotation: its time, the bytes it must move (g and u read, the image written; the A^T fragments are
re-read by every workgroup from cache and not counted) and that rate as a fraction of the HBM peak (benchlib.workloads.HBM_PEAK_GBS).
Not part of bench.py.  Needs a GPU: there is no fall-back.

--decode: the decode step (profiles/gated_decode.json).  Leg A = torch's activation (silu + mul: two launches; relu: one) + forward(), whose
decode route is ONE launch: today's default at these sizes; leg B = forward_gated with decode_gated switched on (lqer_linear_decode_gated:
ONE launch, h formed inside csrc/decode1_kernel.h).  Cases: the Llama-7B down projection (11008 -> 4096, rank 32, silu * up) at M = 1, 2, 4,
6 and OPT-6.7B's fc2 (16384 -> 4096, rank 32, relu, with bias) at M = 1, 4 - the largest M are the last whose LDS image fits.  A launch
streams ~25 MB of weights in ~10 us, so the default --rotate is 16 copies (past the Infinity Cache) and a round times 64 x rotate calls.
`fused_slower` marks a row where leg B's FASTEST round lies above leg A's median, `faster_beyond_spread` one where leg B's slowest round
lies below leg A's fastest: `decode_default` holds, per case, the largest M up to which every row is faster beyond the spread (0: none) -
LinearFlexibleLqer.decode_gated / decode_gated_max_m follow it."""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.hipevents import HipEvent  # noqa: E402
from benchlib.workloads import HBM_PEAK_GBS, MXINT_Q, make_weights  # noqa: E402

K, N, RANK = 11008, 4096, 32
TOKENS = [1, 8, 64, 2048]
EV_FLAGS = 0x20000000  # hipEventDisableSystemFence (benchlib.hipevents)
DEV = "cuda:0"


def _stats(us):
    return {"ms": round(statistics.median(us) / 1e3, 5), "min_ms": round(min(us) / 1e3, 5), "max_ms": round(max(us) / 1e3, 5)}


def _round(calls, stream, e0, e1):
    e0.record(stream)
    for c in calls:
        c()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / len(calls)


def _bytes(M, mod):
    """Algorithmic bytes of the two legs from the shapes: what both move (image written and read, weight, A^T, B^T, y) + the elementwise
    part (leg A: silu reads g writes s, mul reads s and u writes h, the activation side reads h; leg B: g and u read once)."""
    from lqer_amd import _lib

    L, p = _lib.lib(), mod._packed
    Kp = L.lqer_padded_k(K)
    common = 2 * M * Kp * 2 + p["w"].numel() + 2 * L.lqer_padded_r(RANK) * Kp * 2 + L.lqer_padded_r(RANK) * L.lqer_padded_n(N) * 2 + M * N * 2
    return {"torch_silu_mul": 6 * M * K * 2 + common, "forward_gated": 2 * M * K * 2 + common}


DECODE_CASES = {"llama7b_down": dict(K=11008, N=4096, act="silu", up=True, bias=False, q="MXINT_Q", tokens=(1, 2, 4, 6)),
                "opt6.7b_fc2": dict(K=16384, N=4096, act="relu", up=False, bias=True, q="OPT_Q", tokens=(1, 4))}


def _decode(a):
    import benchlib.workloads as WL
    import lqer_amd
    from lqer_amd import ops

    st = ops._stream(torch.device(DEV))
    e0, e1 = HipEvent(EV_FLAGS), HipEvent(EV_FLAGS)
    rows, default = [], {}
    for name, c in DECODE_CASES.items():
        Kc, Nc = c["K"], c["N"]
        W, A, B = make_weights(torch.Generator().manual_seed(11), Kc, Nc, RANK)
        mod = lqer_amd.LinearFlexibleLqer(Kc, Nc, bias=c["bias"], q_config=getattr(WL, c["q"]), l_config={"rank": RANK})
        sd = {"weight": W, "A": A, "B": B}
        if c["bias"]:
            sd["bias"] = 0.1 * torch.randn(Nc, generator=torch.Generator().manual_seed(12))
        mod.load_state_dict(sd)
        mod = mod.to(DEV).half()
        mod.pack()
        mods = [mod] + [copy.deepcopy(mod) for _ in range(a.rotate - 1)]
        for m in mods:
            m.decode_gated, m.decode_gated_max_m = True, 8  # (leg B is the new entry at every size, whatever the defaults keep)
        act_t = torch.nn.functional.silu if c["act"] == "silu" else torch.relu
        for M in c["tokens"]:
            gen = torch.Generator().manual_seed(M)
            gs = [(4 * torch.randn(M, Kc, generator=gen)).half().to(DEV) for _ in range(a.rotate)]
            us = [torch.randn(M, Kc, generator=gen).half().to(DEV) if c["up"] else None for _ in range(a.rotate)]
            legs = {"torch_act": [(lambda m=m, g=g, u=u: m(act_t(g) if u is None else act_t(g) * u)) for m, g, u in zip(mods, gs, us)],
                    "decode_gated": [(lambda m=m, g=g, u=u: m.forward_gated(g, u, c["act"])) for m, g, u in zip(mods, gs, us)]}
            n0 = mods[0].decode_gated_rounds
            ya, yb = legs["torch_act"][0](), legs["decode_gated"][0]()
            assert mods[0].decode_gated_rounds == n0 + 1, "leg B did not take lqer_linear_decode_gated"
            err = float((ya.float() - yb.float()).norm() / ya.float().norm())
            times = {k: [] for k in legs}
            for r in range(2 + a.rounds):
                for k, calls in legs.items():  # (the legs alternate round by round)
                    t = _round(calls * 64, st, e0, e1)
                    if r >= 2:
                        times[k].append(t)
            sa, sb = _stats(times["torch_act"]), _stats(times["decode_gated"])
            row = {"case": name, "M": M, "K": Kc, "N": Nc, "rank": RANK, "act": c["act"], "up": c["up"], "bias": c["bias"],
                   "torch_act": dict(sa, launches=(2 if c["up"] else 1) + 1), "decode_gated": dict(sb, launches=1),
                   "time_ratio": round(sb["ms"] / sa["ms"], 4), "fused_slower": bool(sb["min_ms"] > sa["ms"]),
                   "faster_beyond_spread": bool(sb["max_ms"] < sa["min_ms"]), "rel_l2_between_legs": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del gs, us, legs
        ok = [M for M in c["tokens"] if all(r["faster_beyond_spread"] for r in rows if r["case"] == name and r["M"] <= M)]
        default[name] = max(ok) if ok else 0
        del mods, mod
        torch.cuda.empty_cache()
    doc = {"tool": "tools/gated_mlp_bench.py --decode", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "rotate": a.rotate,
           "note": "per-call times: one HIP event pair around 64 x `rotate` calls of one leg, each on another copy of (g, u) and of the module; "
                   "median / min / max over the rounds, the legs alternating; Python and ctypes included on both legs; launches by construction",
           "decode_default": default, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}: the one-launch entry is faster beyond the spread up to M = {default}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rotate", type=int, default=None)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.rotate = a.rotate or (16 if a.decode else 12)
    a.out = a.out or os.path.join(ROOT, "profiles", "gated_decode.json" if a.decode else "gated_mlp.json")
    assert torch.cuda.is_available(), "needs a GPU"
    if a.decode:
        return _decode(a)
    import lqer_amd
    from lqer_amd import _lib, ops

    W, A, B = make_weights(torch.Generator().manual_seed(11), K, N, RANK)
    mod = lqer_amd.LinearFlexibleLqer(K, N, bias=False, q_config=MXINT_Q, l_config={"rank": RANK})
    mod.load_state_dict({"weight": W, "A": A, "B": B})
    mod = mod.to(DEV).half()
    mod.gated_min_m = 1  # (leg B is the fused entry at every size, whatever the module's default keeps)
    mod.pack()
    mods = [mod] + [copy.deepcopy(mod) for _ in range(a.rotate - 1)]
    st = ops._stream(torch.device(DEV))
    L = _lib.lib()
    e0, e1 = HipEvent(EV_FLAGS), HipEvent(EV_FLAGS)
    rows = []
    for M in TOKENS:
        gen = torch.Generator().manual_seed(M)
        gs = [(4 * torch.randn(M, K, generator=gen)).half().to(DEV) for _ in range(a.rotate)]
        us = [torch.randn(M, K, generator=gen).half().to(DEV) for _ in range(a.rotate)]
        legs = {"torch_silu_mul": [(lambda m=m, g=g, u=u: m(torch.nn.functional.silu(g) * u)) for m, g, u in zip(mods, gs, us)],
                "forward_gated": [(lambda m=m, g=g, u=u: m.forward_gated(g, u)) for m, g, u in zip(mods, gs, us)]}
        # the entry alone, through the C ABI, into one workspace
        desc = mod._desc()
        ws = torch.empty(ops.linear_sizes(desc, M).workspace, dtype=torch.uint8, device=DEV)
        xaq = ws.data_ptr() + (L.lqer_padded_m(M) * L.lqer_padded_k(K) * 2 + 255) // 256 * 256

        def act(m, g, u):
            rc = L.lqer_quantize_act_xa_gated(C.byref(desc), g.data_ptr(), u.data_ptr(), _lib.ACT_SILU, _lib.F16, M, K, K,
                                              m._packed["a_t_b16"].data_ptr(), -2, ws.data_ptr(), xaq, st)
            if rc:
                _lib.check(rc, "quantize_act_xa_gated")

        legs["act_kernel"] = [(lambda m=m, g=g, u=u: act(m, g, u)) for m, g, u in zip(mods, gs, us)]
        ya, yb = legs["torch_silu_mul"][0](), legs["forward_gated"][0]()
        err = float((ya.float() - yb.float()).norm() / ya.float().norm())
        times = {k: [] for k in legs}
        for r in range(2 + a.rounds):
            for k, calls in legs.items():  # (the legs alternate round by round)
                t = _round(calls, st, e0, e1)
                if r >= 2:
                    times[k].append(t)
        sa, sb, sk = (_stats(times[k]) for k in ("torch_silu_mul", "forward_gated", "act_kernel"))
        nb = _bytes(M, mod)
        kb = 2 * M * K * 2 + M * L.lqer_padded_k(K) * 2
        row = {"M": M, "K": K, "N": N, "rank": RANK,
               "torch_silu_mul": dict(sa, launches=2 + (1 if M <= 8 else 2), algorithmic_bytes=nb["torch_silu_mul"]),
               "forward_gated": dict(sb, launches=2, algorithmic_bytes=nb["forward_gated"]),
               "time_ratio": round(sb["ms"] / sa["ms"], 4), "slower_beyond_spread": bool(sb["ms"] > sa["max_ms"]),
               "rel_l2_between_legs": err,
               "act_kernel": dict(sk, bytes=kb, gb_per_s=round(kb / (sk["ms"] * 1e-3) / 1e9, 1),
                                  hbm_fraction=round(kb / (sk["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del gs, us, legs
    doc = {"tool": "tools/gated_mlp_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "rotate": a.rotate,
           "note": "per-call times: one HIP event pair around `rotate` calls of one leg, each on another copy of (g, u) and of the module; "
                   "median / min / max over the rounds, the legs alternating; Python and ctypes included on both legs; act_kernel: "
                   "lqer_quantize_act_xa_gated alone, bytes = g and u read + image written, hbm_fraction against %.0f GB/s" % HBM_PEAK_GBS,
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r["M"] for r in rows if r["slower_beyond_spread"]]
    print(f"wrote {a.out}: forward_gated slower than torch silu + mul + forward beyond the spread at M = {bad or 'no size'}")


if __name__ == "__main__":
    main()

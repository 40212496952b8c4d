"""Time the RMSNorm in front of a shared-input group of a Llama-7B decoder layer together with the group's forward, two ways, in one process:

    leg A   x = HF LlamaRMSNorm(h) as torch launches, then every member's forward on x   (SharedActivation: lqer_quantize_act_xa once +
            one lqer_linear_gemm_ld per member)
    leg B   the group armed with (h, weight, eps), every member's forward on h             (lqer_quantize_act_xa_normed once -
            csrc/act_normed.hip - + the same GEMM calls; x is never written)

    python tools/rmsnorm_bench.py [--rounds 12] [--rotate 6] [--out profiles/rmsnorm_fused.json]

Shapes: the q/k/v group (4096 -> 3 x 4096, rank 32) and the gate/up group (4096 -> 2 x 11008, rank 32), W4A8 MXINT in blocks of 16
(bench.MXINT_Q), fp16, at M = 64, 512, 2048, 8192.
Method: every call of a round works on another of `rotate` copies of h AND of the group's modules (6 x 28 / 50 MB of weight images + up
to 6 x 64 MB of h) so no operand is served from the 256 MB Infinity Cache; 2 warm-up rounds; a round = one HIP event pair
(benchlib.hipevents) around `rotate` calls of one leg, the legs alternating round by round; a row = the median over the rounds with their
spread (min, max).  What is timed is a CALL as a user makes it, Python and ctypes included, on both legs alike.  Per leg also the
launches (by construction: leg A = the 8 torch kernels of the HF formula + the two of the group's quantizer and side product + one
GEMM per member; leg B = 1 + one GEMM per member) and the algorithmic bytes computed from the shapes.  `no_slower` marks a size where
leg B's median is at or below leg A's; LinearFlexibleLqer.normed_min_m is the smallest M from which it holds for both groups at every
larger measured M.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.hipevents import HipEvent  # noqa: E402
from benchlib.workloads import MXINT_Q, make_weights  # noqa: E402

K, RANK, EPS = 4096, 32, 1e-5
GROUPS = {"qkv": (4096, 4096, 4096), "gate_up": (11008, 11008)}
TOKENS = [64, 512, 2048, 8192]
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


def _bytes(M, mods):
    """Algorithmic bytes of the two legs from the shapes: what both move (h read once, the image written once and read by every member's
    GEMM, xaq, weights, A^T, B^T, y) + the norm's own traffic on leg A (the HF formula: h read and an fp32 copy written, that copy read by
    pow and by the multiply, an fp32 product written and read by the cast, x written by the cast, read and written by the weight multiply,
    read by the quantizer: 2 + 4 + 4 + 4 + 4 + 4 + 2 + 2 + 2 + 2 bytes per element beyond leg B's one read of h)."""
    from lqer_amd import _lib

    L = _lib.lib()
    Kp, rp = L.lqer_padded_k(K), sum(L.lqer_padded_r(m.rank) for m in mods)
    common = M * K * 2 + M * Kp * 2 + 2 * M * rp * 2 + 2 * rp * Kp * 2
    for m in mods:
        common += M * Kp * 2 + m._packed["w"].numel() + L.lqer_padded_r(m.rank) * L.lqer_padded_n(m.out_features) * 2 + M * m.out_features * 2
    return {"torch_norm": common + 30 * M * K, "fused_norm": common}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmsnorm_fused.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import lqer_amd
    from lqer_amd import ops
    from lqer_amd.linear import SharedActivation

    lqer_amd.LinearFlexibleLqer.normed_min_m = 1  # (leg B is the fused entry at every size, whatever the default keeps)
    norm = lqer_amd.LinearFlexibleLqer.rms_norm_torch
    st = ops._stream(torch.device(DEV))
    e0, e1 = HipEvent(EV_FLAGS), HipEvent(EV_FLAGS)
    rows = []
    for gname, outs in GROUPS.items():
        protos = []
        for i, N in enumerate(outs):
            W, A, B = make_weights(torch.Generator().manual_seed(11 + i), K, N, RANK)
            m = lqer_amd.LinearFlexibleLqer(K, N, bias=False, q_config=MXINT_Q, l_config={"rank": RANK})
            m.load_state_dict({"weight": W, "A": A, "B": B})
            m = m.to(DEV).half()
            m.pack()
            protos.append(m)
        copies = [[copy.deepcopy(m) for m in protos] for _ in range(a.rotate)]
        groups = [SharedActivation(ms) for ms in copies]
        assert all(g.enabled for g in groups)
        for M in TOKENS:
            gen = torch.Generator().manual_seed(M)
            hs = [torch.randn(M, K, generator=gen).half().to(DEV) for _ in range(a.rotate)]
            ws = [(1 + 0.1 * torch.randn(K, generator=gen)).half().to(DEV) for _ in range(a.rotate)]

            def leg_a(ms, h, w):
                x = norm(h, w, EPS)
                return [m(x) for m in ms]

            def leg_b(g, ms, h, w):
                assert g.normed_serves(h)  # (the question the fused norm module asks before it hands h on)
                g.arm_normed(h, w, EPS)
                return [m(h) for m in ms]

            legs = {"torch_norm": [(lambda ms=ms, h=h, w=w: leg_a(ms, h, w)) for ms, h, w in zip(copies, hs, ws)],
                    "fused_norm": [(lambda g=g, ms=ms, h=h, w=w: leg_b(g, ms, h, w)) for g, ms, h, w in zip(groups, copies, hs, ws)]}
            n0 = groups[0].normed_rounds
            ya, yb = legs["torch_norm"][0](), legs["fused_norm"][0]()
            assert groups[0].normed_rounds == n0 + 1  # leg B really is the normed entry
            err = max(float((p.float() - q.float()).norm() / p.float().norm()) for p, q in zip(ya, yb))
            del ya, yb
            times = {k: [] for k in legs}
            for r in range(2 + a.rounds):
                for k, calls in legs.items():  # (the legs alternate round by round)
                    t = _round(calls, st, e0, e1)
                    if r >= 2:
                        times[k].append(t)
            sa, sb = _stats(times["torch_norm"]), _stats(times["fused_norm"])
            nb = _bytes(M, protos)
            row = {"group": gname, "M": M, "K": K, "N": list(outs), "rank": RANK,
                   "torch_norm": dict(sa, launches=8 + 2 + len(outs), algorithmic_bytes=nb["torch_norm"]),
                   "fused_norm": dict(sb, launches=1 + len(outs), algorithmic_bytes=nb["fused_norm"]),
                   "time_ratio": round(sb["ms"] / sa["ms"], 4), "no_slower": bool(sb["ms"] <= sa["ms"]),
                   "slower_beyond_spread": bool(sb["ms"] > sa["max_ms"]), "max_rel_l2_between_legs": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del hs, ws, legs
        del copies, groups, protos
        SharedActivation.release_pool()
        torch.cuda.empty_cache()
    ok = [M for M in TOKENS if all(r["no_slower"] for r in rows if r["M"] >= M)]
    doc = {"tool": "tools/rmsnorm_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "rotate": a.rotate,
           "note": "per-call times: one HIP event pair around `rotate` calls of one leg, each on another copy of h, the norm weight and the "
                   "group's modules; median / min / max over the rounds, the legs alternating; Python and ctypes included on both legs; "
                   "launches by construction, bytes from the shapes",
           "normed_min_m": min(ok) if ok else None, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}: the fused leg is no slower than torch norm + forward for both groups from M = {doc['normed_min_m']} on")


if __name__ == "__main__":
    main()

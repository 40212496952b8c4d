"""Time the RMSNorm in front of a shared-input group of a Llama-7B decoder layer together with the group's forward, two ways, in one process:

    leg A   x = HF LlamaRMSNorm(h) as torch launches, then every member's forward on x   (SharedActivation: lqer_quantize_act_xa once +
            one lqer_linear_gemm_ld per member)
    leg B   the group armed with (h, weight, eps), every member's forward on h             (lqer_quantize_act_xa_normed once -
            csrc/act_normed.hip - + the same GEMM calls; x is never written)

    python tools/rmsnorm_bench.py [--norm rms|layer] [--rounds 12] [--rotate 6] [--out profiles/rmsnorm_fused.json]

Shapes: the q/k/v group (4096 -> 3 x 4096, rank 32) and the gate/up group (4096 -> 2 x 11008, rank 32), W4A8 MXINT in blocks of 16
(bench.MXINT_Q), fp16, at M = 64, 512, 2048, 8192.
Method: every call of a round works on another of `rotate` copies of h AND of the group's modules (6 x 28 / 50 MB of weight images + up
to 6 x 64 MB of h) so no operand is served from the 256 MB Infinity Cache; 2 warm-up rounds; a round = one HIP event pair
(benchlib.hipevents) around `rotate` calls of one leg, the legs alternating round by round; a row = the median over the rounds with their
spread (min, max).  What is timed is a CALL as a user makes it, Python and ctypes included, on both legs alike.  Per leg also the
launches (by construction: leg A = the 8 torch kernels of the HF formula + the two of the group's quantizer and side product + one
GEMM per member; leg B = 1 + one GEMM per member) and the algorithmic bytes computed from the shapes.  `no_slower` marks a size where
leg B's median is at or below leg A's; LinearFlexibleLqer.normed_min_m is the smallest M from which it holds for both groups at every
larger measured M.  Not part of bench.py.  Needs a GPU: there is no fall-back.

--norm layer: the same for the LayerNorms of an OPT-6.7B layer (profiles/layernorm_fused.json): leg A = F.layer_norm (ONE launch) + the
forward, leg B = the consumer armed with (h, weight, bias, eps) (lqer_quantize_act_xa_layernormed / lqer_linear_forward_layernormed).  The
customers are the q/k/v group (4096 -> 3 x 4096) and fc1 alone (4096 -> 16384; its forward's activation side is one launch from 1024 to
4096 tokens, two elsewhere).  Leg A moves 4 bytes per element beyond leg B: x written by the norm and read by the quantizer.  Each
customer's layer_normed_min_m is the smallest M from which, at that size and every larger one, leg B is not `fused_slower`: its FASTEST
round above leg A's median (slow outliers widen a leg's max with the number of rounds, so the spread is taken on the side that cannot
be noise from other work); None: no such M, the default must never take the fused entry.

--decode: the decode step, M = 1, 4, 8 (profiles/rmsnorm_decode.json, profiles/layernorm_decode.json).  Leg A = torch's norm + the existing
ONE-launch forward (lqer_linear_forward_group / lqer_linear_forward's decode route, csrc/decode1.hip); leg B = the same launch with the
norm formed inside it (lqer_linear_forward_group_normed / lqer_linear_decode_normed and their LayerNorm twins): 1 launch against 9 (RMS)
or 2 (Layer).  --norm rms adds a lone q_proj (4096 -> 4096) as the customer of LinearFlexibleLqer.forward_normed.  A launch streams 9 to
50 MB of weights in ~10 us, so the default --rotate is 16 copies (0.45 to 0.8 GB of weight images: past the Infinity Cache).  Per
customer `decode_default` is False where the fused leg is `fused_slower` at a measured size, else True: the class attributes
decode_normed / decode_layer_normed of linear.SharedActivation (groups) and linear._LinearBase (lone Linears)."""
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
GROUPS = {"rms": {"qkv": (4096, 4096, 4096), "gate_up": (11008, 11008)}, "layer": {"qkv": (4096, 4096, 4096), "fc1": (16384,)}}
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


def _bytes(M, mods, norm_extra):
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
    return {"torch_norm": common + norm_extra * M * K, "fused_norm": common}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--rotate", type=int, default=None)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--norm", choices=("rms", "layer"), default="rms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    layer = a.norm == "layer"
    a.rotate = a.rotate or (16 if a.decode else 6)
    tokens = [1, 4, 8] if a.decode else TOKENS
    customers = dict(GROUPS[a.norm], **({"q_alone": (4096,)} if a.decode and not layer else {}))
    a.out = a.out or os.path.join(ROOT, "profiles", ("layernorm_" if layer else "rmsnorm_") + ("decode.json" if a.decode else "fused.json"))
    assert torch.cuda.is_available(), "needs a GPU"
    import lqer_amd
    from lqer_amd import ops
    from lqer_amd.linear import SharedActivation

    # (leg B is the fused entry at every size, whatever the defaults keep)
    if not a.decode:  # (--decode: the large-M thresholds stay, so a call the one-launch route refuses falls back to torch's norm and is seen)
        lqer_amd.LinearFlexibleLqer.normed_min_m = lqer_amd.LinearFlexibleLqer.layer_normed_min_m = SharedActivation.layer_normed_min_m = 1
    for cls in (lqer_amd.LinearFlexibleLqer, SharedActivation):
        cls.decode_normed = cls.decode_layer_normed = True
    if layer:
        norm = lambda h, wb, eps: torch.nn.functional.layer_norm(h, (K,), wb[0], wb[1], eps)
    else:
        norm = lambda h, wb, eps: lqer_amd.LinearFlexibleLqer.rms_norm_torch(h, wb[0], eps)
    st = ops._stream(torch.device(DEV))
    e0, e1 = HipEvent(EV_FLAGS), HipEvent(EV_FLAGS)
    rows = []
    for gname, outs in customers.items():
        protos = []
        for i, N in enumerate(outs):
            W, A, B = make_weights(torch.Generator().manual_seed(11 + i), K, N, RANK)
            m = lqer_amd.LinearFlexibleLqer(K, N, bias=False, q_config=MXINT_Q, l_config={"rank": RANK})
            m.load_state_dict({"weight": W, "A": A, "B": B})
            m = m.to(DEV).half()
            m.pack()
            protos.append(m)
        copies = [[copy.deepcopy(m) for m in protos] for _ in range(a.rotate)]
        groups = [SharedActivation(ms) if len(ms) > 1 else ms[0] for ms in copies]  # (a lone Linear is its own consumer)
        assert all(g.enabled for g in groups if len(outs) > 1)
        fused_rounds = (lambda g: g.normed_rounds) if len(outs) > 1 else (lambda g: g.layer_normed_rounds if layer else g.decode_normed_rounds)
        for M in tokens:
            gen = torch.Generator().manual_seed(M)
            hs = [torch.randn(M, K, generator=gen).half().to(DEV) for _ in range(a.rotate)]
            ws = [((1 + 0.1 * torch.randn(K, generator=gen)).half().to(DEV), (0.1 * torch.randn(K, generator=gen)).half().to(DEV))
                  for _ in range(a.rotate)]  # (weight, bias: the RMSNorm takes the weight alone)

            def leg_a(ms, h, w):
                x = norm(h, w, EPS)
                return [m(x) for m in ms]

            def leg_b(g, ms, h, w):
                if len(ms) > 1:
                    assert g.normed_serves(h, layer)  # (the question the fused norm module asks before it hands h on)
                if layer:
                    g.arm_layer_normed(h, w[0], w[1], EPS)
                elif len(ms) > 1:
                    g.arm_normed(h, w[0], EPS)
                else:
                    return [g.forward_normed(h, w[0], EPS)]
                return [m(h) for m in ms]

            legs = {"torch_norm": [(lambda ms=ms, h=h, w=w: leg_a(ms, h, w)) for ms, h, w in zip(copies, hs, ws)],
                    "fused_norm": [(lambda g=g, ms=ms, h=h, w=w: leg_b(g, ms, h, w)) for g, ms, h, w in zip(groups, copies, hs, ws)]}
            if a.decode and len(outs) > 1 and not (groups[0].decode_member(copies[0][0], hs[0], hs[0]) is not None and groups[0].normed_serves(hs[0], layer)):
                # (outside the one-launch route on BOTH legs - gate/up at M = 8: more column blocks than one resident round holds)
                rows.append({"group": gname, "M": M, "K": K, "N": list(outs), "rank": RANK, "served": False, "fused_slower": False})
                print(json.dumps(rows[-1]), flush=True)
                continue
            n0 = fused_rounds(groups[0])
            ya, yb = legs["torch_norm"][0](), legs["fused_norm"][0]()
            ran = fused_rounds(groups[0]) == n0 + 1  # leg B really is the normed entry
            if a.decode and not ran:  # (a lone Linear outside the one-launch route - fc1 at M = 8 -: its fused leg fell back to torch's norm)
                rows.append({"group": gname, "M": M, "K": K, "N": list(outs), "rank": RANK, "served": False, "fused_slower": False})
                print(json.dumps(rows[-1]), flush=True)
                continue
            assert ran
            err = max(float((p.float() - q.float()).norm() / p.float().norm()) for p, q in zip(ya, yb))
            del ya, yb
            times = {k: [] for k in legs}
            for r in range(2 + a.rounds):
                for k, calls in legs.items():  # (the legs alternate round by round)
                    t = _round(calls * (64 if a.decode else 1), st, e0, e1)  # (decode: 1024 calls of 12-60 us in a timed window)
                    if r >= 2:
                        times[k].append(t)
            sa, sb = _stats(times["torch_norm"]), _stats(times["fused_norm"])
            nb = _bytes(M, protos, 4 if layer else 30)
            act_side = 2 if len(outs) > 1 or not 1024 <= M <= 4096 else 1  # (launches of the torch leg's quantizer + side product)
            if a.decode:  # (one launch per leg beside the norm's; the image and xaq never reach memory: no byte model)
                la, lb = dict(sa, launches=(1 if layer else 8) + 1), dict(sb, launches=1)
            else:
                la = dict(sa, launches=(1 if layer else 8) + act_side + len(outs), algorithmic_bytes=nb["torch_norm"])
                lb = dict(sb, launches=1 + len(outs), algorithmic_bytes=nb["fused_norm"])
            row = {"group": gname, "M": M, "K": K, "N": list(outs), "rank": RANK, "torch_norm": la, "fused_norm": lb,
                   "time_ratio": round(sb["ms"] / sa["ms"], 4), "no_slower": bool(sb["ms"] <= sa["ms"]),
                   "slower_beyond_spread": bool(sb["ms"] > sa["max_ms"]), "fused_slower": bool(sb["min_ms"] > sa["ms"]),
                   "max_rel_l2_between_legs": err}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del hs, ws, legs
        del copies, groups, protos
        SharedActivation.release_pool()
        torch.cuda.empty_cache()
    if a.decode:  # per customer: on unless the fused leg is slower at a measured size
        key, min_m = "decode_default", {g: not any(r["fused_slower"] for r in rows if r["group"] == g) for g in customers}
    elif layer:  # per customer
        ok = {g: [M for M in TOKENS if not any(r["fused_slower"] for r in rows if r["group"] == g and r["M"] >= M)] for g in GROUPS["layer"]}
        min_m = {g: (min(v) if v else None) for g, v in ok.items()}
    else:
        ok = [M for M in TOKENS if all(r["no_slower"] for r in rows if r["M"] >= M)]
        min_m = min(ok) if ok else None
    doc = {"tool": "tools/rmsnorm_bench.py --norm " + a.norm + (" --decode" if a.decode else ""), "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "rotate": a.rotate,
           "note": "per-call times: one HIP event pair around `rotate` calls of one leg, each on another copy of h, the norm weight and the "
                   "group's modules; median / min / max over the rounds, the legs alternating; Python and ctypes included on both legs; "
                   "launches by construction, bytes from the shapes",
           (key if a.decode else "layer_normed_min_m" if layer else "normed_min_m"): min_m, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}: " + (f"decode defaults {min_m}" if a.decode else f"the fused leg is no slower than torch norm + forward from M = {min_m} on"))


if __name__ == "__main__":
    main()

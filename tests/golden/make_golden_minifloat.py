"""Generate the minifloat golden vectors under tests/golden/ by importing the REFERENCE (read-only, at /root/reference) in the build
container, with make_golden.py's recipe.  Run once, here:  python tests/golden/make_golden_minifloat.py

Only data is written: minifloat.npz (inputs and the reference quantizer's outputs), forward_minifloat.npz + forward_minifloat.json
(LinearFlexible / LinearFlexibleLqer forwards with minifloat in every role, and their configs).  The tests that read them never touch
the reference.
"""
import json
import os
import zlib

import numpy as np
import torch

from make_golden import HERE, bfp_cfg, import_reference

# (width, exponent_width, exponent_bias or None = the reference's default)
FORMATS = [(8, 4, 7), (8, 4, 10), (8, 5, 15), (6, 2, None), (6, 3, None), (4, 2, 1), (4, 2, 7), (4, 1, None), (4, 3, None), (3, 1, None),
           (2, 1, None),
           # exponent ranges up to +127 and down to -119: the floor-log2 rule's largest slacks (|K| >= 64)
           (8, 7, 0), (8, 7, 120)]


def log2_slack(K):
    """d <= slack: torch's fp32 log2 of 2^K (1 - d 2^-24) rounds to K (common.h floor_log2_rule)."""
    q = abs(K).bit_length() - 1 - (1 if K > 0 and K & (K - 1) == 0 else 0)
    return 0 if K == 0 or q < 0 else int(np.ldexp(np.float32(0.6931472), q))


def fmt_key(f):
    return f"{f[0]}_{f[1]}_{'d' if f[2] is None else f[2]}"


def bias_of(f):
    return 2 ** (f[1] - 1) - 1 if f[2] is None else f[2]


def edge_vectors(f):
    """powers of two with their +-1, +-2 ulp neighbours, binade tops, the subnormal binade, RNE ties, saturation, zero / 1e-8 edges."""
    w, ew, _ = f
    m, b = w - ew - 1, bias_of(f)
    emax = 2**ew - 1 - b
    v = []
    for k in range(max(-b - m - 3, -125), min(emax + 3, 128)):
        # the floor-log2 rule's boundary just below 2^k: d = slack and slack + 1 ulps of the binade below (and one less)
        s = log2_slack(k)
        v += [np.float32(2.0**k * (1 - d * 2.0**-24)) for d in (s - 1, s, s + 1, s + 2) if d >= 1]
        p = np.float32(2.0**k)
        v.append(p)
        lo, hi = p, p
        for _ in range(2):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
            v += [lo, hi]
        # the binade's top half-step: above the largest code 2^k (2 - 2^-m), below 2^(k+1)
        top = np.float32(2.0**k * (2 - 2.0 ** -(m + 1)))
        v += [top, np.nextafter(top, np.float32(0)), np.nextafter(top, np.float32(np.inf)), np.float32(2.0**k * (2 - 2.0**-m))]
    # every value of the format and the ties between neighbours (round half to even), plus a point a quarter step on either side
    vals = [2.0 ** (1 - b) * S / 2**m if E == 0 else 2.0 ** (E - b) * (1 + S / 2**m) for E in range(2**ew) for S in range(2**m)]
    for a, c in zip(vals[:-1], vals[1:]):
        v += [np.float32(a), np.float32((a + c) / 2), np.float32(a + (c - a) / 4), np.float32(a + 3 * (c - a) / 4)]
    v += [np.float32(vals[-1]), np.float32(vals[-1] * 1.5), np.float32(vals[-1] * 4), np.float32(1e30), np.finfo(np.float32).max]
    # the subnormal binade [2^-b, 2^(1-b)) and below
    v += list((np.linspace(0.0, 2.0 ** (1 - b), 37, dtype=np.float64)).astype(np.float32))
    t8 = np.float32(1e-8)
    v += [np.float32(0), np.float32(1e-9), t8, np.nextafter(t8, np.float32(0)), np.nextafter(t8, np.float32(1))]
    v = np.array(v, dtype=np.float32)
    v = v[np.isfinite(v)]
    return np.concatenate([v, -v])


def main():
    get_cls, get_q = import_reference()
    mf = get_q("minifloat")
    bfp = get_q("block_fp")
    g = {}
    for f in FORMATS:
        key = fmt_key(f)
        torch.manual_seed(zlib.crc32(key.encode()) % 10000)
        b = bias_of(f)
        emax = 2 ** f[1] - 1 - b
        rnd = torch.randn(4096) * torch.exp2(torch.randint(max(-b - 3, -120), min(emax + 3, 125), (4096,)).float())
        x = torch.cat([torch.from_numpy(edge_vectors(f)), rnd])
        y = mf(x.clone(), f[0], f[1], f[2])
        g[f"{key}/x"], g[f"{key}/y"] = x.numpy(), y.numpy()
        g[f"{key}/fmt"] = np.array([f[0], f[1], b], dtype=np.int64)
        # fp16 inputs: the reference's modules evaluate in the tensor's dtype; this project upcasts to fp32 first
        x16 = x.clamp(-60000.0, 60000.0).half()
        y16 = mf(x16.clone(), f[0], f[1], f[2]).float()
        y32 = mf(x16.float(), f[0], f[1], f[2])
        g[f"{key}/x16"], g[f"{key}/y16_ref"], g[f"{key}/y16_fp32"] = x16.numpy(), y16.numpy(), y32.numpy()
        g[f"{key}/n_fp16_diff"] = np.array([int((y16 != y32).sum())])
    np.savez_compressed(os.path.join(HERE, "minifloat.npz"), **g)
    print("minifloat.npz:", len(g), "arrays")

    def mfc(w, ew, eb):
        return dict(name="minifloat", width=w, exponent_width=ew, exponent_bias=eb)

    base = dict(name="flexible_lqer", is_ptq=True, default=False, x_quantizer=bfp_cfg(8, [1, 16], True), w_quantizer=bfp_cfg(4, [1, 16], False),
                b_quantizer=bfp_cfg(8, [-1], False))
    x8, w4 = mfc(8, 4, 7), mfc(4, 2, 7)
    abq = dict(name="block_fp", width=8, exponent_width=8, exponent_bias=None, block_size=[16, 1], skip_first_dim=False)
    cases = [
        # name, x shape, K, N, r, bias, q_config, A/B quantizer
        ("x_only", (7, 176), 176, 160, 32, True, dict(base, x_quantizer=x8, A_out_quantizer=bfp_cfg(8, [1, 16], True),
                                                      B_out_quantizer=bfp_cfg(8, [1, 16], True)), None),
        ("w_only", (9, 256), 256, 96, 32, False, dict(base, w_quantizer=w4), None),
        ("w_only_e3", (2, 5, 192), 192, 64, 16, True, dict(base, w_quantizer=mfc(4, 3, 8)), None),
        ("fallback", (12, 192), 192, 112, 32, True, dict(base, x_quantizer=x8, w_quantizer=w4, b_quantizer=mfc(8, 4, 10)), None),
        ("all_roles", (2, 35, 128), 128, 160, 16, False, dict(base, x_quantizer=x8, w_quantizer=w4, b_quantizer=mfc(8, 5, 15),
                                                              A_out_quantizer=mfc(8, 5, 15), B_out_quantizer=mfc(8, 4, 10)), None),
        ("ragged", (5, 72), 72, 40, 16, True, dict(base, x_quantizer=mfc(6, 3, None), w_quantizer=w4, A_out_quantizer=mfc(6, 2, None),
                                                   B_out_quantizer=mfc(8, 4, 7)), None),
        ("bfp_ab", (70, 128), 128, 96, 32, True, dict(base, x_quantizer=x8, w_quantizer=w4), abq),
        ("bout_only", (9, 64), 64, 48, 16, False, dict(base, B_out_quantizer=mfc(8, 4, 10)), abq),
    ]
    fw = {}
    for name, xs, K, N, r, has_b, qc, abc in cases:
        torch.manual_seed(zlib.crc32(name.encode()) % 10000)
        x = torch.randn(*xs)
        x.view(-1, K)[:, 7] *= 30.0  # an outlier channel
        W = 0.02 * torch.randn(N, K)
        bias = 0.01 * torch.randn(N) if has_b else None
        wc = qc["w_quantizer"]
        wq = get_q(wc["name"])(W.clone(), **{k: v for k, v in wc.items() if k != "name"})
        U, S, Vh = torch.linalg.svd((W - wq).t().double(), full_matrices=False)
        A, Bm = U[:, :r].float().contiguous(), (S[:r, None] * Vh[:r]).float().contiguous()
        if abc is not None:
            kw = {k: v for k, v in abc.items() if k != "name"}
            A, Bm = bfp(A, **kw), bfp(Bm, **kw)
        mod = get_cls("linear", qc)(K, N, bias=has_b, q_config=qc, l_config={"rank": r})
        with torch.no_grad():
            mod.weight.copy_(W)
            if has_b:
                mod.bias.copy_(bias)
            mod.A.copy_(A)
            mod.B.copy_(Bm)
            y = mod(x)
            xq = mod.x_quantizer(x)
            xAq = mod.A_out_quantizer(torch.matmul(xq, mod.A))
        fw[f"{name}/x"], fw[f"{name}/W"], fw[f"{name}/A"], fw[f"{name}/B"] = x.numpy(), W.numpy(), A.numpy(), Bm.numpy()
        if has_b:
            fw[f"{name}/bias"], fw[f"{name}/bq"] = bias.numpy(), mod.bias.detach().numpy()
        fw[f"{name}/wq"], fw[f"{name}/xq"], fw[f"{name}/xAq"], fw[f"{name}/y"] = mod.weight.detach().numpy(), xq.numpy(), xAq.numpy(), y.numpy()
    # LinearFlexible (no side path)
    flex = dict(base, name="flexible", x_quantizer=x8, w_quantizer=w4, b_quantizer=mfc(8, 4, 10))
    torch.manual_seed(77)
    x = torch.randn(6, 96)
    mod = get_cls("linear", flex)(96, 48, bias=True, q_config=flex, l_config=None)
    W, b = mod.weight.detach().clone(), mod.bias.detach().clone()
    with torch.no_grad():
        y = mod(x)
    fw["flex/x"], fw["flex/W"], fw["flex/bias"], fw["flex/y"] = x.numpy(), W.numpy(), b.numpy(), y.numpy()
    np.savez_compressed(os.path.join(HERE, "forward_minifloat.npz"), **fw)
    cfgs = {c[0]: {"q_config": c[6], "rank": c[4], "bias": c[5]} for c in cases}
    cfgs["flex"] = {"q_config": flex, "rank": 0, "bias": True}
    with open(os.path.join(HERE, "forward_minifloat.json"), "w") as fh:
        json.dump(cfgs, fh, indent=1)
    print("forward_minifloat.npz:", len(fw), "arrays")


if __name__ == "__main__":
    main()

"""Records what the ACTIVATION side launches - Q_x(x), x A and A_out in front of every GEMM - into tests/golden/act_launches.json,
which tests/test_act_launches_cpu.py holds every later library to.  No GPU: tests/launch_probe.cpp (mode `act`) stands in for the HIP
runtime.

    LQER_AMD_LIB=<liblqer_hip.so of the commit to record> python tests/golden/make_golden_act_launches.py

Per format set, K and rank of tests/test_sizes_cpu.py (one N: this side does not read it; three more ranks - 96, 160, 256 - for the
rank-tile counts 3, 5 and 8 of the side GEMM, which RANKS does not reach) and per token count - TOKENS plus 8192 and 16384, where the
staged kernels and the two-window prefetch start - every a_limbs of (1, 2, 3, -1, -2) x pointers (x aligned with
ldx = K; x off by 2 bytes with ldx = K + 1; for LQER_Q_PASSTHROUGH_F16 also xq == x) x scratch (ample; exactly
lqer_lowrank_xa_scratch_bytes; none).  The element type and the tuning bit (none or one of the four this side reads) rotate with the
token count and a_limbs.  Each case makes four calls (launch_probe.cpp): kernels by symbol, grid, workgroup, LDS bytes and the
sizing arguments a grid does not pin, the stream copies of a 5..8-bit weight's wide image, and every refusal with its text.  The
record keeps one digest per descriptor."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_sizes_cpu as G  # noqa: E402
from make_golden_launches import build_probe  # noqa: E402,F401

PATH = os.path.join(HERE, "act_launches.json")
PINS = ("ACT16_SPLIT", "ACT16_FUSED", "ACT8_SPLIT", "ACT8_FUSED")
A_LIMBS = (1, 2, 3, -1, -2)
TOKENS = G.TOKENS + [8192, 16384]
RANKS = G.RANKS + (96, 160, 256)
N = 1000
CUS = 256  # (asked on one path only: lqer_quantize_act_xa_prep plans the GEMM call that follows an int8 activation)


def cases():
    """(descriptor labels, lines per descriptor, the probe's input)."""
    from lqer_amd import _lib

    pins = [0] + [getattr(_lib, "TUNE_" + p) for p in PINS]
    dtypes = (_lib.F16, _lib.BF16, _lib.F32)
    none = _lib.QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
    labels, per, text = [], [], []
    fmt = lambda f: f"{f.kind} {f.width} {f.block} {f.exp_width} {f.exp_bias}"
    for name, fx, fw, fa, fb in G._fmt_sets():
        ptrs = (0, 1, 2) if fx.kind == _lib.Q_PASSTHROUGH_F16 else (0, 1)
        fmts = " ".join(fmt(f) for f in (fx, fw, none, fa, fb))
        for K in G.KS:
            for r in RANKS:
                labels.append(f"{name} K={K} N={N} rank={r}")
                per.append(len(TOKENS) * len(A_LIMBS) * len(ptrs) * 3)
                for i, m in enumerate(TOKENS):
                    for j, al in enumerate(A_LIMBS):  # (i + j runs through all 15 pairs of tuning bit and element type)
                        head = f"{K} {N} {r} {pins[(i + j) % 5]} {fmts} {m} {dtypes[(i + j) % 3]} {al}"
                        text += [f"{head} {p} {s}" for p in ptrs for s in (0, 1, 2)]
    return labels, per, "\n".join(text) + "\n"


def record(lib_path, exe):
    """{descriptor label: digest of its launches}, and the launches themselves per label."""
    labels, per, text = cases()
    out = subprocess.run([exe, lib_path, str(CUS), "act"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == sum(per), (len(out), sum(per))
    lines, at = {}, 0
    for lab, n in zip(labels, per):
        lines[lab] = out[at:at + n]
        at += n
    return {lab: hashlib.sha1("\n".join(v).encode()).hexdigest()[:16] for lab, v in lines.items()}, lines


if __name__ == "__main__":
    from lqer_amd import _lib

    with tempfile.TemporaryDirectory() as tmp:
        digests, lines = record(_lib.LIB_PATH, build_probe(tmp))
    with open(PATH, "w") as f:
        json.dump(digests, f, indent=0)
        f.write("\n")
    ok = sum(" -> 0" in ln for v in lines.values() for ln in v)
    print(PATH, os.path.getsize(PATH), "bytes; library", _lib.LIB_PATH, "; cases with a call that went through:", ok, "of", sum(map(len, lines.values())))
    if len(sys.argv) > 1:  # the launches in full, for a diff between two libraries
        with open(sys.argv[1], "w") as f:
            f.write("".join(f"{lab}\n" + "\n".join(v) + "\n" for lab, v in lines.items()))

"""Records what lqer_linear_gemm_ld launches over the descriptor grid of tests/test_sizes_cpu.py - every kernel by symbol, grid,
workgroup and LDS bytes, the sizing of the B_out pre-pass, and every refusal with its text - into tests/golden/launches.json, which
tests/test_launches_cpu.py holds every later library to.  No GPU: tests/launch_probe.cpp stands in for the HIP runtime.

    LQER_AMD_LIB=<liblqer_hip.so of the commit to record> python tests/golden/make_golden_launches.py

Per descriptor and token count three calls - (fp16, 1 limb of B, no pin), (bf16, 2 limbs, one LQER_TUNE_* bit) and (fp32, 3 limbs,
another bit), the bits rotating with the token count - answered for a device of 256 CUs and for one of 64 (the in-launch exchange of
the row maxima asks the count).  The record keeps one digest per descriptor."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_sizes_cpu as G  # noqa: E402

PATH = os.path.join(HERE, "launches.json")
PINS = ("TILE_ROWS_128", "TILE_ROWS_64", "I8_ROWS_128", "I8_ROWS_256", "AMAX_ATOMIC", "AMAX_PARTS", "AMAX_NO_MRX", "BOUT_IN_PROLOGUE")
CUS = (256, 64)


def build_probe(tmp):
    exe = os.path.join(tmp, "launch_probe")
    subprocess.run(["c++", "-O1", "-std=c++17", "-rdynamic", os.path.join(os.path.dirname(HERE), "launch_probe.cpp"), "-ldl", "-o", exe], check=True)
    return exe


def cases():
    """(descriptor labels, lines per descriptor, the probe's input)."""
    from lqer_amd import _lib

    pins = [getattr(_lib, "TUNE_" + p) for p in PINS]
    labels, text = [], []
    fmt = lambda f: f"{f.kind} {f.width} {f.block} {f.exp_width} {f.exp_bias}"
    for name, d in G._grid():
        labels.append(f"{name} K={d.in_features} N={d.out_features} rank={d.rank}")
        fmts = " ".join(fmt(f) for f in (d.x_fmt, d.w_fmt, d.b_fmt, d.a_out_fmt, d.b_out_fmt))
        for i, m in enumerate(G.TOKENS):
            for dtype, bl, tune in ((_lib.F16, 1, 0), (_lib.BF16, 2, pins[i % len(pins)]), (_lib.F32, 3, pins[(i + 3) % len(pins)])):
                text.append(f"{d.in_features} {d.out_features} {d.rank} {tune} {fmts} {m} {dtype} {bl}")
    return labels, 3 * len(G.TOKENS), "\n".join(text) + "\n"


def record(lib_path, exe):
    """{descriptor label: digest of its launches}, and the launches themselves per label."""
    labels, per, text = cases()
    outs = [subprocess.run([exe, lib_path, str(c)], input=text, capture_output=True, text=True, check=True).stdout.splitlines() for c in CUS]
    assert all(len(o) == per * len(labels) for o in outs), [len(o) for o in outs]
    lines = {lab: [f"cus={c}:{ln}" for c, o in zip(CUS, outs) for ln in o[i * per:(i + 1) * per]] for i, lab in enumerate(labels)}
    return {lab: hashlib.sha1("\n".join(v).encode()).hexdigest()[:16] for lab, v in lines.items()}, lines


if __name__ == "__main__":
    from lqer_amd import _lib

    with tempfile.TemporaryDirectory() as tmp:
        digests, lines = record(_lib.LIB_PATH, build_probe(tmp))
    with open(PATH, "w") as f:
        json.dump(digests, f, indent=0)
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes; library", _lib.LIB_PATH)
    if len(sys.argv) > 1:  # the launches in full, for a diff between two libraries
        with open(sys.argv[1], "w") as f:
            f.write("".join(f"{lab}\n" + "\n".join(v) + "\n" for lab, v in lines.items()))

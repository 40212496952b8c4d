"""Records what the ATTENTION side launches - the two quantized products and the twelve fused attention entries - into
tests/golden/attn_launches.json, which tests/test_attn_launches_cpu.py holds every later library to.  No GPU: tests/launch_probe.cpp
(mode `attn`) stands in for the HIP runtime.

    LQER_AMD_LIB=<liblqer_hip.so of the commit to record> python tests/golden/make_golden_attn_launches.py

Per call: every launch by kernel symbol (i.e. the instantiation), grid, workgroup and dynamic LDS bytes - the image kernels of
kv_cache.hip where a cache or pool call launches them, the standalone quantizer's where a product has a block that is not 16 -, the
value of the entry's *_workspace_bytes function, the return code and every refusal with its text.  The host code of these entries
never dereferences a device pointer (no entry had to be left out): the pointers are fake, 256 MiB apart; caches, pools and
workspaces have the size the library's own functions give.

lqer_matmul_q: blocks of x and of y 16 and 32 (x_pre / y_pre) x y contiguous along j and along k x K in (8, 16, 24, 64, 128, 136, 256)
- below 16, a multiple of 16 and not, Kp <= 128 and beyond - x S2 in (100, 896, 1024) - S2p / 128 of 1, 7 and 8, the k_qmatmul_xr rule -
x S1 in (1, 129); the element type, the batch (1, 2) and the alignment of x and y (each 16-byte aligned or off by one element) rotate.
The attention entries: head dim in (16, 64, 80, 128; 24 and 144 are refused) x heads / kv_heads 4/4 and 8/2 (and for the paged
entries x k_fmt / v_fmt as LQER_Q_MXINT or LQER_Q_MXINT_C4) make a FAMILY; inside it S (0, 1, 8, 9, 129; with per-sequence counts the
bound max_s in (1, 8, 9) x total 0 or positive) x T or max_len (1, 255, 256, 257, 2048, 2049) x mask (none, a tensor with aligned rows,
with rows off by one, the causal rule; paged: none or causal) x window (0, 1, 17; the entries that have one) x n_groups (1, batch; the
shared entry), with the element type, the batch (1, 3) and the alignment of q rotating.  Per family also: batch 0, a workspace one
byte short, no q_strides, formats with blocks of 32.  One digest per family; the record also keeps the sorted kernel symbols reached.

Every kernel of matmul_q.o, attn_q.o and attn_decode.o of the plain build is reached (166 symbols; tools/codeobj_diff.py --kernels
--by-symbol lists them): none is named here as unreachable."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden_launches import build_probe  # noqa: E402,F401

PATH = os.path.join(HERE, "attn_launches.json")
CUS = 256  # (no entry of this side asks)
DS = (16, 64, 80, 128, 24, 144)
HEADS = ((4, 4), (8, 2))
SS = (0, 1, 8, 9, 129)
MAX_S = (1, 8, 9)
TS = (1, 255, 256, 257, 2048, 2049)
WS = (0, 1, 17)
DENSE = ("attention_q", "attention_q_decode", "attention_q_decode_kv", "attention_q_kv")
PAGED = ("attention_q_decode_paged", "attention_q_decode_paged_window", "attention_q_decode_paged_shared", "attention_q_decode_paged_ragged",
         "attention_q_paged", "attention_q_paged_window", "attention_q_paged_ragged", "attention_q_paged_ragged_window")
WINDOWED = ("attention_q_decode_paged_window", "attention_q_decode_paged_ragged", "attention_q_paged_window", "attention_q_paged_ragged_window")


def cases():
    """(family labels, lines per family, the probe's input)."""
    from lqer_amd import _lib

    dtypes = (_lib.F16, _lib.BF16, _lib.F32)
    labels, per, text = [], [], []

    def family(label, lines):
        labels.append(label), per.append(len(lines)), text.extend(lines)

    for xb in (16, 32):
        for yb in (16, 32):
            for lay in (0, 1):
                lines, i = [], 0
                for K in (8, 16, 24, 64, 128, 136, 256):
                    for S2 in (100, 896, 1024):
                        for S1 in (1, 129):
                            for dt in dtypes:  # (i runs through the four alignments and, half as fast, the two batches)
                                lines.append(f"matmul_q {dt} {1 + i // 4 % 2} {S1} {K} {S2} {xb} {yb} {lay} {i % 2} {i // 2 % 2} 0")
                                i += 1
                lines += [f"matmul_q {dtypes[0]} 0 129 64 1024 {xb} {yb} {lay} 0 0 0", f"matmul_q {dtypes[1]} 2 0 64 1024 {xb} {yb} {lay} 0 0 0",
                          f"matmul_q {dtypes[2]} 2 129 64 1024 {xb} {yb} {lay} 0 0 1"]
                family(f"matmul_q x_block={xb} y_block={yb} y_layout={'jk'[lay]}", lines)

    M, C4 = _lib.Q_MXINT, _lib.Q_MXINT_C4
    for name in DENSE + PAGED:
        paged, ragged = name in PAGED, "ragged" in name
        for D in DS:
            for heads, kvh in HEADS:
                for kk, vk in ((M, M), (C4, M), (M, C4), (C4, C4)) if paged else ((M, M),):
                    lines = []

                    def line(S, T, mask, W=0, total=0, groups=1, batch=None, ws=0, nulls=0, blk=16, dt=0, j=0):
                        b = (1, 3)[j % 2] if batch is None else batch
                        lines.append(f"{name} {dtypes[dt % 3]} {b} {heads} {kvh} {S} {T} {D} {mask} {j // 2 % 2} {ws} {nulls} {blk} {kk} {vk} {W} "
                                     f"{total * b} {groups if groups == 1 else b}")

                    # (the element type rotates over S and T - every instantiation's three come up -, batch and alignment over all axes)
                    for si, S in enumerate(MAX_S if ragged else SS):
                        for ti, T in enumerate(TS):
                            for mi, mask in enumerate((0, 3) if paged else (0, 1, 2, 3)):
                                for wi, W in enumerate(WS if name in WINDOWED else (0,)):
                                    for oi, total in enumerate((0, S) if ragged else (0,)):
                                        for gi, groups in enumerate((1, 0) if "shared" in name else (1,)):
                                            line(S, T, mask, W, total, groups, dt=si + ti, j=si + ti + mi + wi + oi + gi)
                    for extra in (dict(batch=0), dict(ws=1), dict(nulls=1), dict(blk=32)):
                        line(1, 257, 3, 17, 1, **extra)
                    kinds = f" k_fmt={kk} v_fmt={vk}" if paged else ""
                    family(f"{name} D={D} heads={heads}/{kvh}{kinds}", lines)
    return labels, per, "\n".join(text) + "\n"


def record(lib_path, exe):
    """{family label: digest of its launches}, the launches themselves per label, the sorted kernel symbols reached."""
    labels, per, text = cases()
    out = subprocess.run([exe, lib_path, str(CUS), "attn"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == sum(per), (len(out), sum(per))
    lines, at = {}, 0
    for lab, n in zip(labels, per):
        lines[lab] = out[at:at + n]
        at += n
    kernels = sorted({m for ln in out for m in re.findall(r"(?:^| )(_Z\w+) \d+,\d+,\d+ ", ln)})
    return {lab: hashlib.sha1("\n".join(v).encode()).hexdigest()[:16] for lab, v in lines.items()}, lines, kernels


if __name__ == "__main__":
    from lqer_amd import _lib

    with tempfile.TemporaryDirectory() as tmp:
        digests, lines, kernels = record(_lib.LIB_PATH, build_probe(tmp))
    with open(PATH, "w") as f:
        json.dump({"digests": digests, "kernels": kernels}, f, indent=0)
        f.write("\n")
    ok = sum(" -> 0" in ln for v in lines.values() for ln in v)
    print(PATH, os.path.getsize(PATH), "bytes; library", _lib.LIB_PATH, "; kernels reached:", len(kernels), "; cases that went through:", ok, "of",
          sum(map(len, lines.values())))
    if len(sys.argv) > 1:  # the launches in full, for a diff between two libraries
        with open(sys.argv[1], "w") as f:
            f.write("".join(f"{lab}\n" + "\n".join(v) + "\n" for lab, v in lines.items()))

"""Records what the composed FORWARD does with a call - lqer_linear_sizes, lqer_linear_forward, lqer_linear_forward_narrow (with
lqer_linear_forward_narrow_workspace_bytes and lqer_weight_narrow_route), lqer_linear_gemm_narrow, lqer_linear_gemm_prepared and
lqer_linear_forward_group (with lqer_group_workspace_bytes) - into tests/golden/fwd_launches.json, which
tests/test_fwd_launches_cpu.py holds every later library to.  No GPU: tests/launch_probe.cpp (mode `fwd`) stands in for the HIP
runtime.

    LQER_AMD_LIB=<liblqer_hip.so of the commit to record> python tests/golden/make_golden_fwd_launches.py

Single Linears: the descriptor grid and TOKENS of tests/test_sizes_cpu.py, and five format sets more over the same K, N and ranks
(the grid has no 2- or 3-bit weight, no integer weight and no block-16 descriptor with a pass-through B_out: the compact image, the
two's-complement nibbles and the second B_out form of the one-launch decode kernel).  One case per descriptor and token count; its
variants - a_limbs of (1, 2, 3, -1, -2), element type, b_limbs, has_bias, pointers (x aligned with ldx = K; x off by 2 bytes with
ldx = K + 1; for LQER_Q_PASSTHROUGH_F16 also xq == x in the split calls) and workspace (exactly the size function's value, twice as
often as: one byte less; null) - are the digits of a multiplicative hash of the case's number, so that every token count meets every
variant over the descriptors; the tuning pin (none or one LQER_TUNE_* bit) rotates with the token count.  Groups: every combination of
1..5 members x M of (0, 1, 8, 9) x a_limbs of (1, 2) x equal / unequal K x equal formats (both B_out forms) or a member whose x, A_out
or B_out format differs x padded ranks that sum to 64, 128 and 144 x pointer (aligned, off by 2 bytes) x workspace (exact, one byte
short, off by 8 bytes) x one member's flaw (none, null w_packed, has_bias without bias_q, rank = -1), and per such kind of group
the calls that are inside the route but for their workspace, at M of (1, 2, 3, 5, 8).

Per call (launch_probe.cpp): the kernels by symbol, grid, workgroup, LDS bytes and sizing arguments, the stream calls, WHERE every
pointer lies (operand+offset: the carving), the return code and the refusal's text; answered for a device of 256 CUs and for one of
64.  The record keeps one digest per label - (format set, K, rank) over the four N, or one kind of group."""
import hashlib
import itertools
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

PATH = os.path.join(HERE, "fwd_launches.json")
PINS = ("TILE_ROWS_128", "TILE_ROWS_64", "I8_ROWS_128", "I8_ROWS_256", "AMAX_ATOMIC", "AMAX_PARTS", "AMAX_NO_MRX", "BOUT_IN_PROLOGUE",
        "ACT16_SPLIT", "ACT16_FUSED", "ACT8_SPLIT", "ACT8_FUSED", "W_EXP_TABLE", "NO_KSPLIT", "DECODE_NO_POLL")
A_LIMBS = (1, 2, 3, -1, -2)
B_LIMBS = (1, 2, 3, 0)
WS = (0, 1, 0, 2)
CUS = (256, 64)


def _fmt(f):
    return f"{f.kind} {f.width} {f.block} {f.exp_width} {f.exp_bias}"


def _extra_sets():
    """(name, x, w, a_out, b_out) format sets the grid of tests/test_sizes_cpu.py does not have."""
    from lqer_amd import _lib
    from lqer_amd._lib import QFmt

    mx = lambda w, blk: QFmt(_lib.Q_MXINT, w, blk, 8, 127)
    pt = lambda w: QFmt(_lib.Q_PASSTHROUGH, w, 0, 8, 127)
    return [
        ("mxint16-w2", mx(8, 16), mx(2, 16), mx(8, 16), mx(8, 16)),       # the compact image, width 2 ...
        ("mxint16-w3-boutpass", mx(8, 16), mx(3, 32), mx(8, 16), pt(0)),  # ... width 3, B_out pass-through
        ("mxint16-w3-bout64", mx(8, 16), mx(3, -1), mx(8, 16), mx(8, 64)),  # ... on a route that reads standard panels at every M
        ("mxint16-boutpass", mx(8, 16), mx(4, 16), mx(8, 16), pt(0)),     # the one-launch decode kernel's second B_out form
        ("mxint16-wint4", mx(8, 16), QFmt(_lib.Q_INT, 4, -1, 1, 3), mx(8, 16), mx(8, 16)),  # signed integer weight, 3 fraction bits
    ]


def _digits(c, *radices):
    """The digits of a multiplicative hash of the case number c."""
    h = (c * 2654435761 & 0xFFFFFFFF) >> 4
    out = []
    for r in radices:
        h, v = divmod(h, r)
        out.append(v)
    return out


def _single_cases(_lib):
    pins = [0] + [getattr(_lib, "TUNE_" + p) for p in PINS]
    dtypes = (_lib.F16, _lib.BF16, _lib.F32)
    none = _lib.QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
    labels, per, text = [], [], []
    c = 0
    for name, fx, fw, fa, fb in G._fmt_sets() + _extra_sets():
        nptr = 3 if fx.kind == _lib.Q_PASSTHROUGH_F16 else 2
        fmts = " ".join(_fmt(f) for f in (fx, fw, none, fa, fb))
        for K in G.KS:
            for r in G.RANKS:
                labels.append(f"{name} K={K} rank={r}")
                per.append(len(G.NS) * len(G.TOKENS))
                for N in G.NS:
                    for i, m in enumerate(G.TOKENS):
                        al, dt, ws, bl, bias, p = _digits(c, 5, 3, 4, 4, 2, nptr)
                        text.append(f"f {K} {N} {r} {bias} {pins[(i + c // len(G.TOKENS)) % len(pins)]} {fmts} {m} {dtypes[dt]} {A_LIMBS[al]} "
                                    f"{B_LIMBS[bl]} {p} {WS[ws]}")
                        c += 1
    return labels, per, text


def _group_cases(_lib):
    from lqer_amd._lib import QFmt

    mx = lambda w, blk: QFmt(_lib.Q_MXINT, w, blk, 8, 127)
    none = QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
    base = (mx(8, 16), mx(4, 16), mx(8, 16), mx(8, 16))
    passb = base[:3] + (none,)
    # (label, the members' formats, the formats of the LAST member: equal, or its x / A_out / B_out format differs)
    odd = (("equal", base, base), ("equal with B_out pass-through", passb, passb), ("x differs", base, (mx(7, 16),) + base[1:]),
           ("A_out differs", base, base[:2] + (mx(6, 16), base[3])), ("B_out differs", base, passb))
    # ranks per member count whose padded values sum to 64 (or about), 128 and 144 (one and two members: with a rank above the kernel's 64)
    ranks = {64: {1: (64,), 2: (32, 32), 3: (16, 20, 32), 4: (16, 16, 16, 16), 5: (16, 16, 16, 8, 8)},
             128: {1: (128,), 2: (64, 64), 3: (64, 32, 32), 4: (32, 32, 32, 32), 5: (32, 32, 32, 16, 16)},
             144: {1: (144,), 2: (80, 64), 3: (48, 48, 48), 4: (48, 32, 32, 32), 5: (32, 32, 32, 32, 16)}}
    dtypes = (_lib.F16, _lib.BF16, _lib.F32)
    labels, per, text = [], [], []
    c = 0
    for n, (oname, base, ofmts), rsum in itertools.product((1, 2, 3, 4, 5), odd, (64, 128, 144)):
        labels.append(f"group of {n}, formats {oname}, ranks {'+'.join(map(str, ranks[rsum][n]))}")
        at = len(text)
        # every combination of what can put a call outside the route, then calls that are inside it but for the workspace
        combos = itertools.chain(itertools.product((0, 1, 8, 9), (1, 2), (0, 1), (0, 1), (0, 1, 2), (0, 1, 2, 3)),
                                 itertools.product((1, 2, 3, 5, 8), (1,), (0,), (0,), (0, 0, 0, 1, 2), (0,)))
        for M, al, kvar, xoff, ws, flaw in combos:
            dt, pin, blv, biasv, who = _digits(c, 3, 3, 8, 2, n)
            c += 1
            line = f"g {n} {M} {dtypes[dt]} {al} {xoff} {ws}"
            for i in range(n):
                K = 1024 if not (kvar and i == n - 1) else 512   # unequal in_features: the last member's
                f = ofmts if i == n - 1 else base
                fmts = " ".join(_fmt(q) for q in (f[0], f[1], none, f[2], f[3]))
                tune = _lib.TUNE_DECODE_NO_POLL if pin == 1 else 0
                bias = 1 if flaw == 2 and i == who else (biasv + i) % 2
                bl = 0 if blv == 7 and i == who else 1 + (blv + i) % 3   # (one case in eight: a member without limbs of B)
                line += f"  {K} {(256, 1000, 48, 4096, 512)[i]} {ranks[rsum][n][i]} {bias} {tune} {fmts} {bl} {flaw if i == who else 0}"
            text.append(line)
        per.append(len(text) - at)
    return labels, per, text


def cases():
    """(labels, lines per label, the probe's input)."""
    from lqer_amd import _lib

    parts = [_single_cases(_lib), _group_cases(_lib)]
    return sum((p[0] for p in parts), []), sum((p[1] for p in parts), []), "\n".join(sum((p[2] for p in parts), [])) + "\n"


def record(lib_path, exe):
    """{label: digest of its calls}, and the calls themselves per label."""
    labels, per, text = cases()
    assert len(set(labels)) == len(labels)
    outs = [subprocess.run([exe, lib_path, str(c), "fwd"], input=text, capture_output=True, text=True, check=True).stdout.splitlines() for c in CUS]
    assert all(len(o) == sum(per) for o in outs), ([len(o) for o in outs], sum(per))
    lines, at = {}, 0
    for lab, n in zip(labels, per):
        lines[lab] = [f"cus={c}:{ln}" for c, o in zip(CUS, outs) for ln in o[at:at + n]]
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
    if len(sys.argv) > 1:  # the calls in full, for a diff between two libraries
        with open(sys.argv[1], "w") as f:
            f.write("".join(f"{lab}\n" + "\n".join(v) + "\n" for lab, v in lines.items()))

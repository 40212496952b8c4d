#!/usr/bin/env python3
"""Device code of two builds, kernel by kernel: codeobj_diff.py [--kernels] [--by-symbol] OBJDIR_A OBJDIR_B  (make OBJDIR=...; no GPU needed).
For every X.o of either directory: the gfx950 code object's FUNC / OBJECT symbols (name, size), each function's disassembly with
addresses (pc-relative distances to global variables included) stripped, and the amdhsa.kernels notes (registers, LDS, scratch, kernarg size) must be equal.  Exit status 1 if not.
--kernels: one line per differing kernel (its symbol: template arguments as I..E) - instruction count A/B and the notes that differ - instead of the first eight
differences of a file.
--by-symbol: functions are paired by symbol across all objects of a directory instead of file by file - for a change that moves kernels to another .hip file."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout


def device_code(obj, tmp):
    fat, co = os.path.join(tmp, "f.fat"), os.path.join(tmp, "f.co")
    if ".hip_fatbin" not in run(f"{LLVM}/llvm-readelf", "-S", "-W", obj):
        return {}, {}, {}  # (host code only)
    run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    syms = {}
    for ln in run(f"{LLVM}/llvm-readelf", "-s", "-W", co).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and not f[7].startswith("__hip_cuid_"):
            syms[f[7]] = (f[3], f[2])
    code, name = {}, None
    for ln in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", ln)
        if m:
            name = m.group(1)
        elif name and ln.strip() not in ("", "..."):  # ("...": the padding behind the last function)
            ins = re.sub(r"\s*// [0-9A-Fa-f]+:.*$|<[^>]*\+0x[0-9a-f]+>", "", ln).strip()
            # the low half of a pc-relative address (s_getpc_b64, then s_add_u32 with the distance to a global variable as a literal): an
            # address like the others - it moves whenever a function between the two changes its size
            if code.get(name) and code[name][-1].startswith("s_getpc_b64"):
                ins = re.sub(r"^(s_add_u32 s\d+, s\d+), 0x[0-9a-f]+$", r"\1, <pc-relative>", ins)
            code.setdefault(name, []).append(ins)
    notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
    keys = r"\.(\w*gpr_count|\w*_spill_count|\w+_segment_\w*size|max_flat_workgroup_size|uses_dynamic_stack):\s+(\S+)"
    meta = {m.group(1): sorted(re.findall(keys, blk)) for blk in notes.split("  - .") if (m := re.search(r"\.name:\s+(\S+)", blk))
            and ".kernarg_segment_size" in blk}
    return syms, code, meta


def per_kernel(A, B):
    """One line per function whose code or notes differ: instruction count A/B, then every note as key A/B that is not equal."""
    names = sorted(k for k in set(A[1]) | set(B[1]) | set(A[2]) | set(B[2]) if A[1].get(k) != B[1].get(k) or A[2].get(k) != B[2].get(k))
    for k in names:
        na, nb = dict(A[2].get(k, ())), dict(B[2].get(k, ()))
        notes = [f"{key} {na.get(key, '-')}/{nb.get(key, '-')}" for key in sorted(set(na) | set(nb)) if na.get(key) != nb.get(key)]
        print(f"  {k}: instructions {len(A[1].get(k, ()))}/{len(B[1].get(k, ()))}; " + (", ".join(notes) if notes else "notes equal"))


def whole_build(d):
    """The device code of every X.o of a directory as one: a kernel that moved to another file keeps its symbol."""
    S, C, M = {}, {}, {}
    for o in sorted(f for f in os.listdir(d) if f.endswith(".o")):
        with tempfile.TemporaryDirectory() as t:
            s, c, m = device_code(os.path.join(d, o), t)
        assert not (set(c) & set(C)), f"{d}/{o}: functions of an earlier object again: {sorted(set(c) & set(C))[:4]}"
        S.update(s), C.update(c), M.update(m)
    return S, C, M


def main(a, b, kernels=False, by_symbol=False):
    if by_symbol:
        A, B = whole_build(a), whole_build(b)
        diff = [f"{what} {k}" for what, x, y in zip(("symbol", "code", "notes"), A, B) for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)]
        only = sorted(set(A[2]) ^ set(B[2]))
        print(f"all objects: {len(A[2])}/{len(B[2])} kernels, {len(only)} in one build only" + "".join(f"\n  only in {'A' if k in A[2] else 'B'}: {k}" for k in only)
              + ": " + ("identical" if not diff else "DIFFERENT: " + "; ".join(diff[:8])))
        if kernels and diff:
            per_kernel(A, B)
        return 1 if diff else 0
    bad = 0
    for o in sorted({f for d in (a, b) for f in os.listdir(d) if f.endswith(".o")}):
        pa, pb = os.path.join(a, o), os.path.join(b, o)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            with tempfile.TemporaryDirectory() as t:
                only = device_code(pa if os.path.exists(pa) else pb, t)
            kernels = len(only[2])
            print(f"{o}: in one build only, {kernels} kernels")
            bad += kernels > 0
            continue
        with tempfile.TemporaryDirectory() as t:
            A, B = device_code(pa, t), device_code(pb, t)
        diff = [f"{what} {k}" for what, x, y in zip(("symbol", "code", "notes"), A, B) for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)]
        assert len(A[1]) >= len(A[2]), f"{o}: {len(A[1])} functions disassembled for {len(A[2])} kernels"
        print(f"{o}: {len(A[0])} symbols, {len(A[1])} functions, {len(A[2])} kernels: " + ("identical" if not diff else "DIFFERENT: " + "; ".join(diff[:8])))
        if kernels and diff:
            per_kernel(A, B)
        bad += bool(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x not in ("--kernels", "--by-symbol")]
    sys.exit(main(args[0], args[1], kernels="--kernels" in sys.argv[1:], by_symbol="--by-symbol" in sys.argv[1:]))

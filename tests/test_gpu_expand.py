"""tests/expand_probe.hip on the GPU: the 4-bit weight expands of lqer_amd/csrc/common.h, every packed byte value in every byte
position times every exponent byte a weight image can hold, against values computed on the host - the gate for the two undocumented
properties of v_cvt_scalef32_pk_bf16_fp8 that the table-free expand (expand_frag_lin) rests on, and for the table forms that images with
exponent bytes beyond it fall back to.  Zero mismatches.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import os
import shutil
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_expand_is_exact_over_all_nibbles_and_exponent_bytes(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "expand_probe")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe, os.path.join(HERE, "expand_probe.hip")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.endswith("mismatches")]
    assert len(lines) == 3 and all(l.endswith(": 0 mismatches") for l in lines), r.stdout
    assert "expand_frag_lin: exponent bytes 1..245" in lines[0] and "1..254" in lines[1] and "1..254" in lines[2]

"""What the fused GEMM launches, no GPU: for every descriptor of the grid of tests/test_sizes_cpu.py x tokens x (element type, limbs of
B, tuning pin) x two device sizes - the kernels of lqer_linear_gemm_ld by symbol (i.e. the instantiation), their grids, workgroups and
LDS bytes, whether a zero fill and which pre-pass run in front and how the pre-pass is sized, and every refusal with its text -
held equal to the record tests/golden/launches.json, which tests/golden/make_golden_launches.py wrote from the library before the
launch plan (csrc/gemm_plan.hip) replaced the hand-kept copies of these decisions.  tests/launch_probe.cpp stands in for the HIP
runtime: one small host program, built here, run once per device size."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_launches_equal_the_record(tmp_path):
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    spec = importlib.util.spec_from_file_location("make_golden_launches", os.path.join(GOLDEN, "make_golden_launches.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    with open(R.PATH) as f:
        gold = json.load(f)
    digests, lines = R.record(_lib.LIB_PATH, R.build_probe(str(tmp_path)))
    assert list(digests) == list(gold)
    for label, want in gold.items():
        assert digests[label] == want, f"{label}: the launches differ from the record; this library's:\n" + "\n".join(lines[label][:12])
    assert sum(" -> 0" in ln for v in lines.values() for ln in v) > 100000  # (most of the grid launches; the rest are refusals)

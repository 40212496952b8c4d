"""What the activation side launches, no GPU: for every format set, K and rank of the grid of tests/test_sizes_cpu.py x tokens x
(a_limbs, element type, tuning pin) x pointer / stride variant x scratch variant - the kernels of lqer_quantize_act_xa (with xaq,
without, and as lqer_quantize_act_xa_prep) and of lqer_lowrank_xa by symbol (i.e. the instantiation), their grids, workgroups, LDS
bytes and sizing arguments (the split-K plan, the staged kernels' chunks, the padded rank, k_quant_xa16's vector flag, the zero fill
of k_act8_fused), the stream copies behind a 5..8-bit weight, *ready_bytes, and every refusal with its text - held equal to the record
tests/golden/act_launches.json, which tests/golden/make_golden_act_launches.py wrote from the library before the side path's file
(csrc/lowrank_xa.hip) was split by kernel family and its dispatch decisions were each written once.  tests/launch_probe.cpp (mode
`act`) stands in for the HIP runtime."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_act_launches_equal_the_record(tmp_path):
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    spec = importlib.util.spec_from_file_location("make_golden_act_launches", os.path.join(GOLDEN, "make_golden_act_launches.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    with open(R.PATH) as f:
        gold = json.load(f)
    digests, lines = R.record(_lib.LIB_PATH, R.build_probe(str(tmp_path)))
    assert list(digests) == list(gold)
    for label, want in gold.items():
        assert digests[label] == want, f"{label}: the launches differ from the record; this library's:\n" + "\n".join(lines[label][:12])
    # 472298 of the 814275 cases of the recorded run have a call that goes through (the rest: no scratch, a rank of 0 for the side
    # GEMM, a form the descriptor does not take - all refusals, with their texts in the record)
    assert sum(" -> 0" in ln for v in lines.values() for ln in v) > 450000

"""What the composed forward does with a call, no GPU: lqer_linear_sizes, lqer_linear_forward, lqer_linear_forward_narrow (with its
workspace size and lqer_weight_narrow_route), lqer_linear_gemm_narrow, lqer_linear_gemm_prepared and lqer_linear_forward_group (with
lqer_group_workspace_bytes) over the descriptor grid of tests/test_sizes_cpu.py, five format sets more and the group cases of
tests/golden/make_golden_fwd_launches.py - the kernels by symbol, grid, workgroup, LDS bytes and sizing arguments, the stream calls,
where every pointer a kernel or stream call receives lies in the caller's buffers (operand+offset: the carving of the workspace), the
size functions' values, the return codes and every refusal with its text - held equal to the record tests/golden/fwd_launches.json,
which that script wrote from the library before the forward's host code (csrc/api.hip) got one carving, one decode rule, one fill of
the per-call kernel arguments and its format check by role.  tests/launch_probe.cpp (mode `fwd`) stands in for the HIP runtime."""
import importlib.util
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# what the record must reach at least once, or it could pass while empty: (what, pattern in the calls' full text)
FAMILIES = (
    ("k_decode1 with one member", r"k_decode1ILi\dELi\dELb0E"),
    ("k_decode1 with a group", r"k_decode1ILi\dELi\dELb1E"),
    ("k_decode1, B_out pass-through", r"k_decode1ILi\dELi0E"),
    ("k_decode1, B_out in blocks of 16", r"k_decode1ILi\dELi1E"),
    ("k_decode1_narrow at width 2", r"k_decode1_narrowILi\dELi\dELi2E"),
    ("k_decode1_narrow at width 3", r"k_decode1_narrowILi\dELi\dELi3E"),
    ("the small-M kernel summing partial tiles", r"k_lqer_gemm_smallm\S* \S+ \S+ \S+ \{[^}]* xa_part=ws\+"),
    ("the small-M kernel on the compact image", r"k_lqer_gemm_smallm_narrowI"),
    ("the 128-row tile kernel", r"4lqer11k_lqer_gemmI"),
    ("the 256-row tile kernel", r"k_lqer_gemm_m256I"),
    ("the int8 kernel", r"k_lqer_gemm_i8I"),
    ("k_act16_fused", r"k_act16_fusedI"),
    ("k_act8_fused", r"k_act8_fusedI"),
    ("the weight-widen kernel into the workspace", r"k_w_widen\S* \S+ \S+ \S+ \{ in=w\+0 out=ws\+"),
    ("the weight-widen kernel into widen_scratch", r"k_w_widen\S* \S+ \S+ \S+ \{ in=w\+0 out=widen\+0"),
    ("the replicate copy behind a 5..8-bit weight", r"hipMemcpy2DAsync \d+ \d+ \d+ \d+ \{ dst=ws\+0 src=ws\+"),
    ("x itself as the image", r"k_lqer_gemm\S* \S+ \S+ \S+ \{ xq=x\+0 "),
    ("LQER_NARROW_DIRECT", r" route=1 "),
    ("LQER_NARROW_DIRECT_ONE_LAUNCH", r" route=2 "),
    ("LQER_NARROW_WIDEN", r" route=3 "),
)


def test_fwd_launches_equal_the_record(tmp_path):
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    spec = importlib.util.spec_from_file_location("make_golden_fwd_launches", os.path.join(GOLDEN, "make_golden_fwd_launches.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    with open(R.PATH) as f:
        gold = json.load(f)
    digests, lines = R.record(_lib.LIB_PATH, R.build_probe(str(tmp_path)))
    assert list(digests) == list(gold)
    for label, want in gold.items():
        assert digests[label] == want, f"{label}: the calls differ from the record; this library's:\n" + "\n".join(lines[label][:12])
    # 215878 of the 277350 cases of the recorded run have a call that goes through (the rest: a workspace one byte short or null in
    # every call of the case, a form the descriptor does not take, a group outside the route - all refusals, with their texts in
    # the record)
    assert sum(" -> 0" in ln for v in lines.values() for ln in v) > 200000
    full = "\n".join(ln for v in lines.values() for ln in v)
    for what, pattern in FAMILIES:
        assert re.search(pattern, full), f"the cases reach no call with {what}"

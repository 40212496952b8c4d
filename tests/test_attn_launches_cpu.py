"""What the attention side launches, no GPU: for lqer_matmul_q and the twelve lqer_attention_q* entries, over the smallest values on
either side of every decision their dispatch makes (tests/golden/make_golden_attn_launches.py lists them) - the kernels by symbol (i.e.
the instantiation), their grids, workgroups and LDS bytes, the image kernels a cache or pool call puts in front, the value of the
entry's *_workspace_bytes function, the return code and every refusal with its text - held equal to the record
tests/golden/attn_launches.json, which the recorder wrote from the library before the launch ladders of csrc/matmul_q.hip,
csrc/attn_q.hip and csrc/attn_decode.hip were each written once.  tests/launch_probe.cpp (mode `attn`) stands in for the HIP runtime."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_attn_launches_equal_the_record(tmp_path):
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    spec = importlib.util.spec_from_file_location("make_golden_attn_launches", os.path.join(GOLDEN, "make_golden_attn_launches.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    with open(R.PATH) as f:
        gold = json.load(f)
    digests, lines, kernels = R.record(_lib.LIB_PATH, R.build_probe(str(tmp_path)))
    assert list(digests) == list(gold["digests"])
    for label, want in gold["digests"].items():
        assert digests[label] == want, f"{label}: the launches differ from the record; this library's:\n" + "\n".join(lines[label][:12])
    # every kernel of matmul_q.o, attn_q.o and attn_decode.o (166), the image kernels of kv_cache.hip and the standalone quantizer's
    assert kernels == gold["kernels"]
    # 18500 of the 61512 cases of the recorded run go through (the rest: S beyond the split kernels' 8 rows, head dims 24 and 144, a window
    # without the causal rule or of 0 keys, nibble codes on the grouped entry, short workspaces, ... - refusals, their texts in the record)
    assert sum(" -> 0" in ln for v in lines.values() for ln in v) >= 18500

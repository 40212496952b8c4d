"""The host decisions of the fused GEMM, no GPU: route, tile rows (refusals included), GEMM scratch bytes and the decode-partials
answer over the descriptor grid of tests/test_sizes_cpu.py x tokens x element type x tile pins, held equal - no exceptions - to the
record tests/golden/routes.json (tests/golden/make_golden_routes.py wrote it from the library before the launch plan of
csrc/gemm_plan.hip replaced the hand-kept copies of these decisions)."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_routes", os.path.join(GOLDEN, "make_golden_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_decisions_equal_the_record(lib):
    R = _recorder()
    with open(R.PATH) as f:
        gold = json.load(f)
    assert gold["tokens"] == list(R.G.TOKENS) and gold["columns"] == R.columns()
    n = 0
    for (label, got), row in zip(R.walk(lib), gold["desc"], strict=True):
        want = [gold["series"][i] for i in gold["rows"][row]]
        if got != want:
            for col, g, w in zip(gold["columns"], got, want):
                for m, a, b in zip(gold["tokens"], R.unrle(g), R.unrle(w)):
                    assert a == b, f"{label} M={m}: {col} = {a}, the record says {b}"
            assert got == want, f"{label}: the series differ from the record in length or encoding"
        n += 1
    assert n == len(gold["desc"]) == 1600

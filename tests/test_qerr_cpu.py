"""Host side of lqer_qerr_matmul (include/lqer_hip.h "quantization-error products") and of lqer_factors' `method`, no GPU: the export,
the workspace size, and the refusals - every check of the entry point runs before its first launch."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lqer_amd import _lib, ops  # noqa: E402
from lqer_amd.approximate import approximate_model, lqer_factors  # noqa: E402

MX16 = _lib.QFmt(_lib.Q_MXINT, 4, 16, 8, 127)
N, K, L = 64, 256, 48


def call(dtype=_lib.F16, fmt=MX16, L=L, ws_bytes=None):
    """lqer_qerr_matmul on addresses that are never touched: the call must refuse before it launches."""
    lib = _lib.lib()
    need = lib.lqer_qerr_matmul_workspace_bytes(N, K, min(max(L, 1), 256), 0)
    rc = lib.lqer_qerr_matmul(4096, dtype, N, K, K, C.byref(fmt) if fmt is not None else None, None, 0, 8192, L, L, 12288, L, 16384,
                              need if ws_bytes is None else ws_bytes, None)
    return rc, lib.lqer_last_error().decode()


def test_export_and_workspace_size():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    lib = _lib.lib()
    for name in ("lqer_qerr_matmul", "lqer_qerr_matmul_workspace_bytes"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr) and getattr(lib, name)
    assert "#define LQER_ABI_VERSION 14" in hdr
    for trans in (0, 1):
        sizes = [lib.lqer_qerr_matmul_workspace_bytes(4096, 11008, l, trans) for l in (1, 8, 48, 144, 256)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.lqer_qerr_matmul_workspace_bytes(N, K, 257, 0) == 0


@pytest.mark.parametrize("kwargs,code,text", [
    (dict(fmt=_lib.QFmt(_lib.Q_MINIFLOAT, 4, -1, 2, 1)), -2, "dense source"),
    (dict(fmt=_lib.QFmt(_lib.Q_MXINT, 4, -1, 8, 127)), -2, "dense source"),   # whole-row blocks
    (dict(L=0), -1, "outside [1,256]"),
    (dict(L=257), -1, "outside [1,256]"),
    (dict(fmt=None), -1, "must be LQER_F32"),
    (dict(ws_bytes=64), -4, "lqer_qerr_matmul_workspace_bytes"),
])
def test_refusals(kwargs, code, text):
    rc, msg = call(**kwargs)
    assert rc == code and text in msg, (rc, msg)


def test_2d_tile_format_is_refused_with_the_dense_source_named():
    cfg = dict(name="block_fp", width=4, exponent_width=8, exponent_bias=None, block_size=[8, 16], skip_first_dim=False)
    with pytest.raises(NotImplementedError, match="dense source"):
        ops.qerr_matmul(torch.zeros(16, 16), cfg, torch.zeros(16, 4), 0)
    assert not ops.qerr_fused_covers(ops.make_qfmt(cfg, "w")) and ops.qerr_fused_covers(MX16)


def test_method_argument():
    assert inspect.signature(lqer_factors).parameters["method"].default == "svd"
    assert inspect.signature(approximate_model).parameters["method"].default == "svd"
    with pytest.raises(ValueError, match="nonsense"):
        lqer_factors(torch.zeros(16, 16), dict(name="block_fp", width=4, block_size=[1, 16]), 4, method="nonsense")

"""A plain `bench.py --dump-outputs DIR` run on the GPU: the JSON line carries the headline alone (no roofline, secondary region,
parity or CPU baseline), and DIR/y.npy holds what the timed C-ABI path computed - its rows meet the CPU oracle on the same
seeded inputs.  Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bench import MXINT_Q, WORKLOADS, make_weights, make_x
    from lqer_amd import sweep
    from oracle import lqer_oracle as O

    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "bf16"
    for k in ("roofline", "module", "uninstrumented", "two_streams", "model_shared_inputs", "group", "parity_rel_l2"):
        assert d[k] is None, k
    assert "configs" not in d and "cpu_baseline" not in d

    y = np.load(out / "y.npy")
    _, M, r, _, qc, shapes, _ = WORKLOADS["c2"]
    K, N, _ = shapes[0]
    assert qc is MXINT_Q and y.dtype == np.float32 and y.shape == (M, N) and np.isfinite(y).all()
    # the runner's operands: x from seed 0, the Linear's weights from rank 0's first unit seed
    x = make_x(M, K, seed=0)[0].half().float()
    W, A, B = make_weights(torch.Generator().manual_seed(sweep.unit_seed(0, 0)), K, N, r, bias=False, quantize_ab=True)
    h = lambda t: t.half().float()
    rows = torch.tensor([0, 1, 777, M - 1])
    ref = O.lqer_linear_forward(x[rows], h(W), None, h(A), h(B), qc)
    got = torch.from_numpy(y[rows.numpy()])
    assert float((got - ref).norm() / ref.norm()) <= 1e-3

"""bench.py's options and its --dump-outputs writer, without a GPU: the plain run is the headline alone (--full adds the rest), and
the dumped arrays are float32, exact when they fit, a seeded row sample of the same rows in every run when they do not, and at
most 64 MB in all."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_plain_and_full_options():
    import pytest

    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    b = bench.parse_args(["--full", "--no-configs", "--dump-outputs", "out"])
    assert b.full and b.no_configs and b.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args(["--warmup", "-1"])


def test_plain_run_opts_time_the_headline_alone():
    """What main() hands run_workload: a plain run turns off every region, check and figure beside the headline; --full turns
    them on, less what the --no-* options leave out; --dump-outputs reaches the runner either way."""
    import bench

    o = bench.run_opts(bench.parse_args(["--workload", "c2", "--steps", "5", "--warmup", "1", "--dump-outputs", "d"]))
    assert (o.workload, o.steps, o.warmup, o.dump) == ("c2", 5, 1, "d")
    assert not (o.full or o.check or o.module or o.two_streams or o.cpu_base or o.uninstrumented)
    f = bench.run_opts(bench.parse_args(["--workload", "c2", "--full"]))
    assert f.full and f.check and f.module and f.two_streams and f.cpu_base and f.uninstrumented and f.dump is None
    t = bench.run_opts(bench.parse_args(["--workload", "c2", "--full", "--no-check", "--no-module", "--no-two-streams",
                                         "--no-cpu-baseline"]))
    assert t.full and t.uninstrumented and not (t.check or t.module or t.two_streams or t.cpu_base)


def test_dump_outputs_exact_and_sampled(tmp_path):
    from benchlib.runner import DUMP_BYTES, dump_outputs

    g = torch.Generator().manual_seed(3)
    small = torch.randn(64, 96, generator=g).half()
    big = [torch.randn(2048, n, generator=g).half() for n in (4096, 11008, 4096)]
    dump_outputs(str(tmp_path / "a"), [("y", small)])
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.dtype == np.float32 and np.array_equal(y, small.float().numpy())

    named = [("y_4096x4096", big[0]), ("y_4096x11008", big[1]), ("y_11008x4096", big[2])]
    dump_outputs(str(tmp_path / "b"), named)
    dump_outputs(str(tmp_path / "c"), named)
    total = 0
    for name, t in named:
        f = tmp_path / "b" / (name + ".npy")
        total += os.path.getsize(f)
        got = np.load(f)
        assert got.dtype == np.float32 and got.shape[1] == t.shape[1] and 0 < got.shape[0] < t.shape[0]
        assert np.array_equal(got, np.load(tmp_path / "c" / (name + ".npy")))  # the same sample in every run
        full = t.float().numpy()
        assert all(any(np.array_equal(row, full[i]) for i in range(full.shape[0])) for row in got[:3])  # rows of the output
    assert total <= DUMP_BYTES <= 64 * 10 ** 6

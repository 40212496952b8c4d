"""The calibration profiler on the host side: the float64 restatement (tests/_calib.py) against the reference's own outputs
(tests/golden/calib.npz / calib.json), the two new entry points across header, binding and library, their argument errors without a
GPU, the hook factories' bookkeeping through the `stats_fn` seam, and approximate_model's "<name>.scale" keys."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import _calib as CB
from lqer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD, META = CB.load_fixture()
CASES = sorted(META["cases"])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_fixture_covers_what_it_should():
    cs = META["cases"].values()
    assert {c["dtype"] for c in cs} == {"float32", "float16"}
    assert {len(c["shape"]) for c in cs} == {2, 3}
    assert {c["shape"][-1] for c in cs} == {50, 100, 768} and {c["rows"] for c in cs} == {1, 37, 1000}
    assert META["thresholds"] == [6.0, 0.5]
    size = sum(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in ("calib.npz", "calib.json"))
    assert size < 1_000_000, size


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    """The reference's stored fp32 outputs sit inside the derived float64 bounds for every case; threshold dictionaries are equal."""
    c = META["cases"][name]
    xs = CB.case_batches(GOLD, META, name)
    M, K = c["rows"], c["shape"][-1]
    s = torch.zeros(K, dtype=torch.float64)
    per_batch = []
    for x in xs:
        per_batch.append(x.double().abs().reshape(-1, K).mean(0))
        s = CB.scale_step(s, x)
    ref_s = torch.from_numpy(GOLD[f"{name}/scales"])
    e = CB.rel_err(ref_s, s)
    print(f"{name}: scales rel err {e:.3e} (bound {CB.bound_scale(M, False):.3e})")
    assert e <= CB.bound_scale(M, False)
    ref_n, want_n = torch.from_numpy(GOLD[f"{name}/scale_dict"]), CB.normalise(s)
    e = CB.rel_err(ref_n, want_n)
    print(f"{name}: normalised rel err {e:.3e} (bound {CB.bound_norm(M, False):.3e})")
    assert e <= CB.bound_norm(M, False)
    # the fixture exercises what it claims: a clamped column, maxima from different batches
    assert bool((s < CB.CLAMP).any())
    assert len({int(i) for i in torch.stack(per_batch).argmax(0).tolist()}) > 1
    clamped = ref_s < CB.CLAMP
    assert bool((ref_n[clamped] == ref_n[clamped][0]).all())
    for t in META["thresholds"]:
        th = c["thresholds"][str(t)]
        counts = [CB.n_cols_ge(x, t) for x in xs]
        assert counts == th["counts"]
        assert {"lin.threshold": CB.threshold_entry(counts, (META["out_features"], K), t, META["seq_len"])} == th["dict"]


def test_symbols_in_header_library_and_binding(lib):
    hdr = open(os.path.join(ROOT, "include", "lqer_hip.h")).read()
    for n in ("lqer_col_abs_stats", "lqer_col_abs_stats_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert re.search(r"#define\s+LQER_ABI_VERSION\s+14\b", hdr) and _lib.ABI_VERSION == 14 and lib.lqer_version() == 14


def test_argument_errors_without_gpu(lib):
    ws = lib.lqer_col_abs_stats_workspace_bytes
    assert ws(8192, 4096) > 0 and ws(1, 50) > 0
    assert ws(8192, 11008) > ws(8192, 4096) > ws(8192, 50)
    assert ws(0, 4096) == 0 and ws(8192, 0) == 0
    assert ws(8192, 4096) <= 8192 * 4096 * 2 // 8  # the partials stay a small fraction of an fp16 x
    f = lib.lqer_col_abs_stats
    x = run = wsp = 0x1000  # never dereferenced: validation comes before any HIP call
    big = ws(64, 128)
    for args in ((None, _lib.F16, 64, 128, 128, run, None, 0.0, None, wsp, big, None),      # null x
                 (x, _lib.F16, 0, 128, 128, run, None, 0.0, None, wsp, big, None),          # M <= 0
                 (x, _lib.F16, 64, 0, 128, run, None, 0.0, None, wsp, big, None),           # K <= 0
                 (x, _lib.F16, -1, 128, 128, run, None, 0.0, None, wsp, big, None),
                 (x, _lib.F16, 64, 128, 127, run, None, 0.0, None, wsp, big, None),         # ldx < K
                 (x, 7, 64, 128, 128, run, None, 0.0, None, wsp, big, None),                # unknown dtype
                 (x, _lib.F16, 64, 128, 128, None, None, 6.0, None, wsp, big, None)):       # no output at all
        assert f(*args) == -1, args
        assert b"col_abs_stats" in lib.lqer_last_error()
    assert f(x, _lib.F16, 64, 128, 128, run, None, 0.0, None, wsp, big - 1, None) == -4
    assert f(x, _lib.F16, 64, 128, 128, run, None, 0.0, None, None, 0, None) == -4
    assert b"workspace" in lib.lqer_last_error()


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=96, max_position_embeddings=64)
    return LlamaForCausalLM(cfg).eval()


def test_hook_keys_match_the_reference():
    from lqer_amd import calibrate

    seq = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))
    fac = calibrate.register_scale_hooks(seq, stats_fn=CB.stats_cpu)
    assert list(fac.scales) == ["0.scale", "2.scale"] and list(fac.is_profiled.values()) == [False, False]
    assert fac.scales["0.scale"].shape == (8,) and fac.scales["0.scale"].dtype == torch.float32
    with pytest.raises(AssertionError, match="Not all scales are profiled"):
        fac.get_scale_dict()
    seq[0](torch.randn(3, 8))  # one hook fired, the other not: still refused
    assert fac.is_profiled == {"0.scale": True, "2.scale": False} and not fac.is_all_profiled()
    with pytest.raises(AssertionError):
        fac.get_scale_dict()
    seq(torch.randn(2, 3, 8))
    assert fac.is_all_profiled() and set(fac.get_scale_dict()) == {"0.scale", "2.scale"}
    tf = calibrate.register_threshold_hooks(seq, 6.0, seq_len=16, stats_fn=CB.stats_cpu)
    assert list(tf.results) == ["0.threshold", "2.threshold"]
    with pytest.raises(AssertionError, match="Not all thresholds are profiled"):
        tf.get_threshold_dict()
    with pytest.raises(ValueError, match="Unknown mode"):
        calibrate.register_scale_hooks(seq, mode="max(abs())")

    model = _tiny_llama()
    fac = calibrate.register_scale_hooks(model, stats_fn=CB.stats_cpu)
    want = [n + ".scale" for n, m in model.named_modules() if isinstance(m, nn.Linear)]
    assert list(fac.scales) == want and "lm_head.scale" in want and "model.layers.1.mlp.down_proj.scale" in want
    assert len(want) == 2 * 7 + 1
    fac.remove_hooks()
    # subclasses of nn.Linear are hooked as well: a model after quantize_model
    from bench import MXINT_Q
    from lqer_amd.models import quantize_model

    quantize_model(model, {"linear": MXINT_Q}, {"linear": {"rank": 16}})
    assert list(calibrate.register_scale_hooks(model, stats_fn=CB.stats_cpu).scales) == want


def test_cpu_tensor_without_stats_fn_raises():
    from lqer_amd import calibrate

    lin = nn.Linear(8, 4)
    calibrate.register_scale_hooks(lin)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lin(torch.randn(2, 8))
    lin = nn.Linear(8, 4)
    calibrate.register_threshold_hooks(lin, 6.0, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lin(torch.randn(2, 8))


@pytest.mark.parametrize("name", CASES)
def test_factory_bookkeeping_against_the_fixture(name):
    """Running maximum across batches, normalisation and threshold dictionaries of the factories, with a torch stand-in for the
    kernel: the reference's stored values within twice the float64 bounds (two fp32 evaluations), dictionaries equal."""
    from lqer_amd import calibrate

    c = META["cases"][name]
    xs = CB.case_batches(GOLD, META, name)
    M, K = c["rows"], c["shape"][-1]
    fac = calibrate.ScaleHookFactoryMeanAbs(stats_fn=CB.stats_cpu)
    hook = fac.get_scale_hook("lin.scale", K)
    for x in xs:
        hook(None, (x,), None)
    assert CB.rel_err(fac.scales["lin.scale"], torch.from_numpy(GOLD[f"{name}/scales"])) <= CB.bound_scale(M, True)
    sd = fac.get_scale_dict()
    assert CB.rel_err(sd["lin.scale"], torch.from_numpy(GOLD[f"{name}/scale_dict"])) <= CB.bound_norm(M, True)
    assert fac.scales["lin.scale"] is sd["lin.scale"]  # (the reference stores the normalised scale back)
    for t in META["thresholds"]:
        tf = calibrate.ThresholdHookFactory(t, seq_len=META["seq_len"], stats_fn=CB.stats_cpu)
        th = tf.get_threshold_hook("lin.threshold", K, META["out_features"])
        for x in xs:
            th(None, (x,), None)
        assert all(torch.is_tensor(v) for v in tf.results["lin.threshold"]["running_num_x_cols_hp"])  # read once, at the end
        assert CB.as_lists(tf.get_threshold_dict()) == c["thresholds"][str(t)]["dict"]


def test_profile_model_runs_batches_and_removes_hooks():
    from lqer_amd import calibrate

    seq = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))
    xs = [torch.randn(5, 8) for _ in range(3)]
    sd = calibrate.profile_model(seq, xs, stats_fn=CB.stats_cpu)
    assert set(sd) == {"0.scale", "2.scale"} and all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd.values())
    s = torch.zeros(8, dtype=torch.float64)
    for x in xs:
        s = CB.scale_step(s, x)
    assert CB.rel_err(sd["0.scale"], CB.normalise(s)) <= CB.bound_norm(5, False)
    assert not seq[0]._forward_hooks and not seq[2]._forward_hooks

    class Two(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(8, 4)

        def forward(self, input_ids, scale=1.0):
            return self.fc(input_ids * scale)

    assert set(calibrate.profile_model(Two(), [{"input_ids": xs[0], "scale": 2.0}], stats_fn=CB.stats_cpu)) == {"fc.scale"}


def test_approximate_model_reads_reference_keys():
    from bench import MXINT_Q
    from lqer_amd import LinearFlexibleLqer
    from lqer_amd.approximate import approximate_model

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = LinearFlexibleLqer(32, 48, bias=False, q_config=MXINT_Q, l_config={"rank": 16})
            self.b = LinearFlexibleLqer(48, 32, bias=False, q_config=MXINT_Q, l_config={"rank": 16})
            self.c = LinearFlexibleLqer(32, 32, bias=False, q_config=MXINT_Q, l_config={"rank": 16})

    seen = {}

    def fake_factors(W, w_cfg, r, a_cfg, b_cfg, scale):
        seen[tuple(W.shape)] = scale
        return torch.zeros(W.shape[1], r), torch.zeros(r, W.shape[0])

    sa, sb, wrong = torch.full((32,), 2.0), torch.full((48,), 3.0), torch.full((32,), 9.0)
    approximate_model(Model(), scale_dict={"a.scale": sa, "a": wrong, "b": sb}, factors_fn=fake_factors)
    assert seen[(48, 32)] is sa      # the reference's key, ahead of the plain name
    assert seen[(32, 48)] is sb      # the plain module name still works
    assert seen[(32, 32)] is None    # missing: plain SVD

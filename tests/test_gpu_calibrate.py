"""The calibration profiler on the GPU: ops.col_abs_stats (csrc/col_stats.hip) and the hook factories against the reference's stored
outputs (tests/golden/calib.npz) and the float64 restatement (tests/_calib.py) within the derived bounds; exact column maxima and
counts; strides, alignment, NaN, determinism, graph replay; profile_model -> approximate_model end to end on a tiny Llama."""
import pytest
import torch
import torch.nn as nn

import _calib as CB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD, META = CB.load_fixture()
CASES = sorted(META["cases"])


def same_bits(a, b):
    return torch.equal(a.float().cpu().view(torch.int32), b.float().cpu().view(torch.int32))


def check_against_f64(x, M=None):
    """one call on a fresh running scale against the float64 restatement; exact maxima and counts"""
    from lqer_amd import ops

    K = x.shape[-1]
    M = M or x.numel() // K
    st = ops.col_abs_stats(x, run=torch.zeros(K, device=x.device), want_absmax=True, threshold=0.5)
    xc = x.cpu()
    want = CB.scale_step(torch.zeros(K, dtype=torch.float64), xc)
    e = CB.rel_err(st.run, want)
    print(f"{tuple(x.shape)} {x.dtype}: rel err {e:.3e} (bound {CB.bound_scale(M, False):.3e})")
    assert e <= CB.bound_scale(M, False)
    assert same_bits(st.absmax, xc.float().abs().reshape(-1, K).amax(0))
    assert int(st.count) == CB.n_cols_ge(xc, 0.5)
    return st


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_through_the_op(name):
    from lqer_amd import ops

    c = META["cases"][name]
    xs = CB.case_batches(GOLD, META, name)
    M, K = c["rows"], c["shape"][-1]
    run = torch.zeros(K, device=DEV)
    s64 = torch.zeros(K, dtype=torch.float64)
    for x in xs:
        for t in META["thresholds"]:
            st = ops.col_abs_stats(x.to(DEV), want_absmax=True, threshold=t)
            assert st.run is None
            assert same_bits(st.absmax, x.float().abs().reshape(-1, K).amax(0))
            assert int(st.count) == CB.n_cols_ge(x, t)
        out = ops.col_abs_stats(x.to(DEV), run=run)
        assert out.run is run and out.absmax is None and out.count is None
        s64 = CB.scale_step(s64, x)
    e_ref, e_64 = CB.rel_err(run, torch.from_numpy(GOLD[f"{name}/scales"])), CB.rel_err(run, s64)
    print(f"{name}: running scale rel err vs reference {e_ref:.3e} (bound {CB.bound_scale(M, True):.3e}), vs float64 {e_64:.3e}")
    assert e_ref <= CB.bound_scale(M, True) and e_64 <= CB.bound_scale(M, False)


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_through_the_factories(name):
    from lqer_amd import calibrate

    c = META["cases"][name]
    xs = [x.to(DEV) for x in CB.case_batches(GOLD, META, name)]
    M, K = c["rows"], c["shape"][-1]
    fac = calibrate.ScaleHookFactoryMeanAbs()
    hook = fac.get_scale_hook("lin.scale", K)
    for x in xs:
        hook(None, (x,), None)
    assert fac.scales["lin.scale"].device.type == "cuda" and fac.scales["lin.scale"].dtype == torch.float32
    assert CB.rel_err(fac.scales["lin.scale"], torch.from_numpy(GOLD[f"{name}/scales"])) <= CB.bound_scale(M, True)
    got = fac.get_scale_dict()["lin.scale"]
    ref_n = torch.from_numpy(GOLD[f"{name}/scale_dict"])
    e = CB.rel_err(got, ref_n)
    print(f"{name}: normalised rel err vs reference {e:.3e} (bound {CB.bound_norm(M, True):.3e})")
    assert e <= CB.bound_norm(M, True)
    clamped = torch.from_numpy(GOLD[f"{name}/scales"]) < CB.CLAMP
    assert bool(clamped.any()) and bool((got.cpu()[clamped] == got.cpu()[clamped][0]).all())
    for t in META["thresholds"]:
        tf = calibrate.ThresholdHookFactory(t, seq_len=META["seq_len"])
        th = tf.get_threshold_hook("lin.threshold", K, META["out_features"])
        for x in xs:
            th(None, (x,), None)
        assert CB.as_lists(tf.get_threshold_dict()) == c["thresholds"][str(t)]["dict"]


def test_bf16_strides_alignment_and_one_row():
    g = torch.Generator().manual_seed(11)
    check_against_f64(torch.randn(300, 520, generator=g).bfloat16().to(DEV))
    check_against_f64(torch.randn(3, 70, 77, generator=g).bfloat16().to(DEV))     # K no multiple of 8: scalar tail group
    wide = torch.randn(257, 1000, generator=g).half().to(DEV)
    check_against_f64(wide[:, 8:648])     # ldx > K, 16-byte aligned rows
    check_against_f64(wide[:, 3:604])     # ldx > K, rows only 2-byte aligned: the scalar variant
    odd = torch.randn(129 * 333 + 1, generator=g).half().to(DEV)[1:].view(129, 333)  # base 2-byte aligned, odd pitch
    check_against_f64(odd)
    w32 = torch.randn(100, 210, generator=g).to(DEV)
    check_against_f64(w32[:, 1:202])      # fp32, rows 4-byte aligned only
    check_against_f64(torch.randn(1, 4096, generator=g).half().to(DEV))           # M = 1
    check_against_f64(torch.randn(1, 50, generator=g).to(DEV))
    # the vector and the scalar variant add in the same order: same bits
    from lqer_amd import ops

    a = ops.col_abs_stats(wide[:, 8:648].contiguous()).run
    shifted = torch.empty(257 * 640 + 1, dtype=torch.float16, device=DEV)[1:].view(257, 640)
    shifted.copy_(wide[:, 8:648])
    assert torch.equal(a, ops.col_abs_stats(shifted).run)


@pytest.mark.parametrize("K", [4096, 11008])
def test_full_size_fp16_and_determinism(K):
    from lqer_amd import ops

    g = torch.Generator(device=DEV).manual_seed(K)
    x = torch.randn(4, 2048, K, generator=g, device=DEV, dtype=torch.float16)
    x[..., 7] *= 50.0
    a = check_against_f64(x)
    b = ops.col_abs_stats(x, run=torch.zeros(K, device=DEV), want_absmax=True, threshold=0.5)
    assert torch.equal(a.run, b.run) and torch.equal(a.absmax, b.absmax) and torch.equal(a.count, b.count)


def test_small_determinism_and_fp32_full_width():
    from lqer_amd import ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(1000, 768, generator=g).to(DEV)
    a, b = check_against_f64(x), ops.col_abs_stats(x, run=torch.zeros(768, device=DEV), want_absmax=True, threshold=0.5)
    assert torch.equal(a.run, b.run) and torch.equal(a.absmax, b.absmax) and torch.equal(a.count, b.count)


def test_nan_column_behaves_like_torch():
    from lqer_amd import ops

    g = torch.Generator().manual_seed(3)
    x = torch.randn(200, 96, generator=g)
    x[17, 5] = float("nan")      # NaN next to values >= threshold: the column still counts (its other elements compare true)
    x[:, 9] = 0.01
    x[3, 9] = float("nan")       # NaN next to small values only: not counted
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        xd = x.to(dt)
        run = torch.full((96,), 0.25)
        st = ops.col_abs_stats(xd.to(DEV), run=run.to(DEV), want_absmax=True, threshold=0.5)
        want_run = torch.maximum(run, xd.float().abs().mean(0))
        want_max = xd.float().abs().amax(0)
        assert torch.isnan(want_run[5]) and torch.isnan(want_max[9])
        assert torch.equal(torch.isnan(st.run.cpu()), torch.isnan(want_run))
        assert torch.equal(torch.isnan(st.absmax.cpu()), torch.isnan(want_max))
        ok = ~torch.isnan(want_max)
        assert torch.equal(st.absmax.cpu()[ok], want_max[ok])
        assert int(st.count) == int((xd.abs() >= 0.5).any(0).sum())
        # a NaN already in the running scale stays (torch.maximum)
        run2 = torch.zeros(96)
        run2[40] = float("nan")
        out = ops.col_abs_stats(xd.to(DEV), run=run2.to(DEV)).run.cpu()
        assert torch.isnan(out[40]) and torch.isnan(out[5]) and not torch.isnan(out[41])


@pytest.mark.parametrize("shape,dt", [((64, 256), torch.float16), ((2048, 4096), torch.float16), ((300, 101), torch.float32)])
def test_graph_replay_matches_eager(shape, dt):
    from lqer_amd import ops
    from lqer_amd.graph import GraphedCallable

    g = torch.Generator().manual_seed(shape[0])
    K = shape[1]
    xs = [torch.randn(*shape, generator=g).to(dt).to(DEV) * (i + 1) for i in range(3)]
    static_x = xs[0].clone()
    run = torch.zeros(K, device=DEV)

    def fn(x):
        st = ops.col_abs_stats(x, run=run, want_absmax=True, threshold=0.5)
        return st.run, st.absmax, st.count

    gc = GraphedCallable(fn, static_x)
    run.zero_()
    eager_run = torch.zeros(K, device=DEV)
    for x in (xs[1], xs[2], xs[0]):
        r, amax, cnt = gc(x)
        e = ops.col_abs_stats(x, run=eager_run, want_absmax=True, threshold=0.5)
        assert torch.equal(r, e.run) and torch.equal(amax, e.absmax) and torch.equal(cnt, e.count)


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=320, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).eval()


def test_profile_then_approximate_on_a_tiny_llama():
    from bench import MXINT_Q
    from lqer_amd import LinearFlexibleLqer, calibrate
    from lqer_amd.approximate import approximate_model, lqer_factors
    from lqer_amd.models import quantize_model

    model = _tiny_llama().to(DEV)
    g = torch.Generator().manual_seed(1)
    batches = [{"input_ids": torch.randint(0, 320, (2, 48), generator=g).to(DEV)} for _ in range(3)]
    # the restated hooks on the same dense model: float64 running maxima from recorded inputs
    want, rows, handles = {}, {}, []
    for name, m in model.named_modules():
        if isinstance(m, nn.Linear):
            def rec(mod, inp, out, key=name + ".scale"):
                x = inp[0].detach().cpu()
                want[key] = CB.scale_step(want.get(key, torch.zeros(x.shape[-1], dtype=torch.float64)), x)
                rows[key] = x.numel() // x.shape[-1]
            handles.append(m.register_forward_hook(rec))
    with torch.no_grad():
        for b in batches:
            model(**b)
    for h in handles:
        h.remove()
    sd = calibrate.profile_model(model, batches)
    assert set(sd) == set(want) and "lm_head.scale" in sd and len(sd) == 15
    for k, v in sd.items():
        assert v.device.type == "cpu" and v.dtype == torch.float32
        assert CB.rel_err(v, CB.normalise(want[k])) <= CB.bound_norm(rows[k], False), k

    a_cfg = b_cfg = dict(name="block_fp", width=8, exponent_width=8, exponent_bias=None, block_size=[16, 1], skip_first_dim=False)

    def factors(scale_dict):
        torch.manual_seed(0)
        m = quantize_model(_tiny_llama().to(DEV), {"linear": MXINT_Q}, {"linear": {"rank": 16}})
        return m, approximate_model(m, a_cfg, b_cfg, scale_dict=scale_dict)

    m1, ab = factors(sd)
    _, ab0 = factors(None)
    n_diff = 0
    for name, mod in m1.named_modules():
        if isinstance(mod, LinearFlexibleLqer):
            ref = _tiny_llama().to(DEV).get_submodule(name)
            A, B = lqer_factors(ref.weight.data, mod.q_config.get("w_quantizer", mod.q_config["default"]), mod.rank, a_cfg, b_cfg,
                                sd[name + ".scale"])
            assert torch.equal(ab[name + ".A"], A.to(mod.A.dtype)) and torch.equal(ab[name + ".B"], B.to(mod.B.dtype)), name
            n_diff += int(not torch.equal(ab[name + ".A"], ab0[name + ".A"]))
    assert n_diff == 14

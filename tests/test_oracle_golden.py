"""The oracle (oracle/lqer_oracle.py) against vectors produced by the reference itself
(tests/golden/make_golden.py).  CPU only; never reads /root/reference."""
import numpy as np
import pytest
import torch

from oracle import lqer_oracle as O


def _qnames(g):
    return sorted({k.split("/")[1] for k in g.files if k.startswith("q/")})


def test_golden_present(golden_q, golden_fwd):
    assert len(_qnames(golden_q)) >= 20
    assert len(golden_fwd[0].files) > 50


@pytest.mark.parametrize("via_unfold", [False, True])
def test_mxint_quantizer_bit_exact(golden_q, via_unfold):
    for name in _qnames(golden_q):
        x = torch.from_numpy(golden_q[f"q/{name}/x"])
        y = torch.from_numpy(golden_q[f"q/{name}/y"])
        meta = golden_q[f"q/{name}/meta"].tolist()
        width, skip, block = meta[0], bool(meta[1]), meta[2:]
        got = O.mxint_quantize(x, width=width, block_size=block, skip_first_dim=skip, via_unfold=via_unfold)
        assert got.dtype == torch.float32 and got.shape == y.shape
        assert torch.equal(got.view(torch.int32), y.view(torch.int32)) or torch.equal(got, y), name


def test_mxint_libm_route_agrees(golden_q):
    """The bit-pattern ceil(log2) rule and torch's own log2 give the same quantizer output."""
    for name in _qnames(golden_q):
        x = torch.from_numpy(golden_q[f"q/{name}/x"])
        meta = golden_q[f"q/{name}/meta"].tolist()
        a = O.mxint_quantize(x, width=meta[0], block_size=meta[2:], skip_first_dim=bool(meta[1]))
        b = O.mxint_quantize(x, width=meta[0], block_size=meta[2:], skip_first_dim=bool(meta[1]), libm_log2=True)
        assert torch.equal(a, b), name


def test_ceil_log2_rule_table(golden_q):
    ks = golden_q["log2_rule/k"]
    slack = golden_q["log2_rule/slack"]
    got = O._slack_ulps(torch.from_numpy(ks)).numpy()
    assert np.array_equal(got, slack)
    # and every neighbour up to 63 ulps
    for k, s in zip(ks.tolist(), slack.tolist()):
        bits = np.uint32((k + 127) << 23) + np.arange(0, 64, dtype=np.uint32)
        v = torch.from_numpy(bits.view(np.float32).copy())
        e = O.ceil_log2_f32(v).numpy()
        want = np.where(np.arange(64) <= s, k, k + 1)
        assert np.array_equal(e, want), k


def test_decompose_consistent(golden_q):
    for name in _qnames(golden_q):
        meta = golden_q[f"q/{name}/meta"].tolist()
        width, skip, block = meta[0], bool(meta[1]), meta[2:]
        x = torch.from_numpy(golden_q[f"q/{name}/x"])
        if x.ndim != 2 or skip is False and block[0] != 1:
            continue
        y, codes, exps = O.mxint_quantize(x, width=width, block_size=block, skip_first_dim=skip, decompose=True)
        L = O.infer_block_shape([1, x.shape[1]], block)[-1]
        e = exps.reshape(x.shape[0], -1).repeat_interleave(L, dim=1)[:, : x.shape[1]].float()
        rebuilt = codes.float() * torch.pow(2.0, e - (width - 1))
        ref = torch.where(x.abs() <= 1e-8, torch.zeros_like(y), y)
        assert torch.equal(rebuilt, ref), name
        assert int(codes.abs().max()) <= 2 ** (width - 1) - 1


def test_integer_quantizer(golden_q):
    for key in [k for k in golden_q.files if k.startswith("int/") and k.endswith("/x")]:
        tag = key.split("/")[1]
        w, f = tag[1:].split("f")
        got = O.integer_quantize(torch.from_numpy(golden_q[key]), int(w), int(f))
        assert torch.equal(got, torch.from_numpy(golden_q[f"int/{tag}/y"]))


FWD_CASES = ["m1", "m7", "m64", "b2s5", "r128", "int128", "introw", "ragged", "a16", "a16row", "a16mix", "intx", "intx70", "tile8", "tileall",
             "w8row", "w8g128", "w8b16", "w6b32",  # (w8*: weights of 5..8 bits, round 5)
             # activation blocks that span token rows (round 5): [R, L] tiles of 3-D tensors, 2-D tensors blocked like a weight
             "acttile3d", "acttile_ragged", "acttile2d", "acttile2d_all", "acttile_r_on_2d", "acttile_whole", "acttile_bout",
             # (round 6) the quantizer's default block_size [16] on a 3-D tensor (all token rows x 16 columns) and on a 2-D one (per row);
             # the W3A16 weight-only sweep (sweep_lqer_act_w-only.sh:74-77): 3-bit weights in blocks of 32, pass-through activations, rank 64
             "acttile_lone3d", "acttile_lone2d", "w3b32_a16_r64", "w3b32_a16_r64_3d"]


@pytest.mark.parametrize("name", FWD_CASES)
def test_forward_matches_reference(golden_fwd, name):
    g, cfgs = golden_fwd
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"])
    bias = t("bias") if f"{name}/bias" in g.files else None
    out = O.lqer_linear_forward(t("x"), t("W"), bias, t("A"), t("B"), cfgs[name], intermediates=True)
    assert torch.equal(out["xq"], t("xq"))
    assert torch.equal(out["wq"], t("wq"))
    if bias is not None:
        assert torch.equal(out["bq"], t("bq"))
    for k in ("xA", "xAq", "xAB", "xABq", "y"):
        ref = t(k)
        err = (out[k] - ref).norm() / ref.norm().clamp_min(1e-30)
        assert err <= 1e-6, (k, float(err))
    # the quantizers applied to the reference's own intermediates are bit exact
    qs = O.resolve_linear_quantizers(cfgs[name])
    assert torch.equal(O.get_quantizer(qs["A_out"])(t("xA")), t("xAq"))
    assert torch.equal(O.get_quantizer(qs["B_out"])(t("xAB")), t("xABq"))


def test_forward_no_side_path(golden_fwd):
    g, cfgs = golden_fwd
    t = lambda k: torch.from_numpy(g[f"flex/{k}"])
    y = O.lqer_linear_forward(t("x"), t("W"), t("bias"), None, None, cfgs["flex"])
    assert (y - t("y")).norm() / t("y").norm() <= 1e-6


@pytest.mark.parametrize("name", ["flex_w8a8_row", "flex_w8a8_g128"])
def test_forward_no_side_path_w8a8(golden_fwd, name):
    """LinearFlexible in the configuration the reference runs it with (sweep_baseline_no_lqer.sh:73-76: W8A8, one block per weight
    row and per token, bias in the activations' format) and with weight blocks of 128: y, the quantized weight and bias."""
    g, cfgs = golden_fwd
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"])
    out = O.lqer_linear_forward(t("x"), t("W"), t("bias"), None, None, cfgs[name], intermediates=True)
    assert torch.equal(out["wq"], t("wq")) and torch.equal(out["bq"], t("bq"))
    assert (out["y"] - t("y")).norm() / t("y").norm() <= 1e-6


def test_pack_unpack_roundtrip(golden_q):
    for name, block in (("w4_b16", 16), ("w4_b128", 128), ("w4_row", -1), ("w4_ragged", 16)):
        x = torch.from_numpy(golden_q[f"q/{name}/x"])
        y = torch.from_numpy(golden_q[f"q/{name}/y"])
        codes, exps = O.pack_weight_mxint4(x, block, n_pad=8, k_pad=64)
        assert codes.dtype == torch.uint8 and exps.dtype == torch.int8
        assert codes.shape[0] % 8 == 0 and (codes.shape[1] * 2) % 64 == 0
        w = O.unpack_weight_mxint4(codes, exps, x.shape[0], x.shape[1], block)
        ref = torch.where(x.abs() <= 1e-8, torch.zeros_like(y), y)  # declared flush, block_fp.py:79-80
        assert torch.equal(w, ref), name


def test_flop_model():
    assert O.flops(2048, 4096, 4096, 32) == 2 * 2048 * 4096 * 4096 + 2 * 2048 * 4096 * 32 + 2 * 2048 * 32 * 4096


def test_oracle_quantized_matmuls_vs_reference_vectors():
    """matmul_flexible / bmm_flexible (quantized_functions/matmul.py) against outputs of the imported reference:
    Q K^T with a transposed second operand whose last dim is not a block multiple, P V, and a 3-D bmm."""
    import json
    import os

    import numpy as np

    here = os.path.join(os.path.dirname(__file__), "golden")
    g = np.load(os.path.join(here, "matmul.npz"))
    qc = json.load(open(os.path.join(here, "matmul_config.json")))
    blk = json.load(open(os.path.join(here, "matmul_config_blocks.json")))  # (round 4) blocks of 32 / one block per row of y
    for name in ("b32", "brow"):
        out = O.matmul_flexible(torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/y"]), blk[name])
        assert torch.equal(out, torch.from_numpy(g[f"{name}/out"])), name
    out = O.matmul_flexible(torch.from_numpy(g["lone/x"]), torch.from_numpy(g["lone/y"]), blk["lone"])  # (round 6: a lone [16] = [1, S, 16] tiles)
    assert float((out - torch.from_numpy(g["lone/out"])).norm() / torch.from_numpy(g["lone/out"]).norm()) <= 1e-6
    for name, fn in (("qk", O.matmul_flexible), ("pv", O.matmul_flexible), ("bmm", O.bmm_flexible)):
        out = fn(torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/y"]), qc)
        assert torch.equal(out, torch.from_numpy(g[f"{name}/out"])), name
    with pytest.raises(KeyError):  # the reference evaluates q_config["default"] eagerly
        O.matmul_flexible(torch.zeros(1, 2, 16), torch.zeros(1, 16, 2), {"name": "flexible", "x_quantizer": qc["x_quantizer"]})


def test_fp16_evaluation_of_the_reference_differs_only_at_small_magnitude_ties():
    """The reference evaluates models in fp16 (runners.py:203): there `+ 1e-9` is a no-op, exact .5 ties round to even and
    log2 is rounded to a half.  This build (oracle and kernels alike) upcasts 16-bit inputs and quantizes in fp32, where
    1e-9 breaks the ties of small values upward.  The vectors of tests/golden/make_golden_fp16.py (the reference run on
    fp16 tensors) put a number on it: activations of unit scale - block_fp 8-bit in blocks of 16 or per token - come out
    identical; LLM-sized weights (sigma 0.02, 4-bit) differ in 0.16 % / 0.04 % of the elements (blocks of 16 / 128), 8-bit
    values of sigma 0.01 in 1.2 %, always by one quantization step; the rates are pinned here."""
    import os

    import numpy as np

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantizers_fp16.npz"))
    bound = {"act8": 0.0, "row8": 0.0, "w4": 0.003, "w4_128": 0.001, "small8": 0.02, "ties8": 0.5}
    for name in sorted({k.split("/")[0] for k in g.files}):
        x, y = torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/y"]).float()
        meta = g[f"{name}/meta"].tolist()
        ours = O.mxint_quantize(x.float(), width=meta[0], block_size=meta[2:], skip_first_dim=bool(meta[1]))
        diff = ours != y
        assert diff.float().mean().item() <= bound[name], (name, diff.float().mean().item())
        # a differing element is one step of its block away, never more
        w = meta[0]
        step = (ours - y).abs()
        assert (step[diff] <= y.abs().max() * 2.0 ** (2 - w) + 1e-12).all(), name


# ---- narrow exponent fields: both clamps of block_fp.py:46-51 active (tests/golden/make_golden_expfield.py) -------------------------
def _expfield():
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantizers_expfield.npz"))


def _expfield_names(g):
    return sorted({k.rsplit("/", 1)[0] for k in g.files})


def _expfield_kw(meta):
    width, ew, has_b, eb, skip = meta[:5]
    return dict(width=width, exponent_width=ew, exponent_bias=eb if has_b else None, block_size=meta[5:], skip_first_dim=bool(skip))


def test_expfield_golden_present_and_clamped():
    """The fixture holds every (format, width) pair of tests/_formats.py, and in every format narrower than fp32 the reference met
    both clamps: each of {clamped at emin, unclamped, clamped at emax} holds at least 15 % of the non-zero blocks."""
    import _formats as F

    g = _expfield()
    names = _expfield_names(g)
    for p in set(F.ACT_PAIRS + F.W4_PAIRS + F.W8_PAIRS):
        assert f"b16/{F.pair_id(p)}" in names
    for kind in ("b128", "row", "tile4x16", "act3d", "act3d_tile"):
        assert any(n.startswith(kind + "/") for n in names), kind
    for name in names:
        fid = name.split("/")[1].split("-")[0]
        kw = _expfield_kw(g[f"{name}/meta"].tolist())
        F.assert_covered(torch.from_numpy(g[f"{name}/x"]), fid, dict(kw, name="block_fp"), torch.float32)


@pytest.mark.parametrize("via_unfold", [False, True])
def test_expfield_quantizer_bit_exact(via_unfold):
    """Every value of the fixture, bit for bit - except the sign of a zero, which this test, like test_mxint_quantizer_bit_exact,
    does not pin: the oracle writes +0 where the reference's sign(x + 1e-9) * 0 leaves -0."""
    g = _expfield()
    for name in _expfield_names(g):
        x, y = torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/y"])
        kw = _expfield_kw(g[f"{name}/meta"].tolist())
        got = O.mxint_quantize(x, **kw, via_unfold=via_unfold)
        assert got.dtype == torch.float32 and got.shape == y.shape
        assert torch.equal(got.view(torch.int32), y.view(torch.int32)) or torch.equal(got, y), name
        assert torch.equal(O.mxint_quantize(x, **kw, libm_log2=True), got), name


def test_expfield_decompose_reconstructs():
    """decompose=True: codes 2^(exponent - mbits) is the quantizer's output (the |x| <= 1e-8 pass-through as 0), the exponents lie
    inside the field's range and the codes inside the width's."""
    g = _expfield()
    for name in _expfield_names(g):
        x = torch.from_numpy(g[f"{name}/x"])
        kw = _expfield_kw(g[f"{name}/meta"].tolist())
        y, codes, exps = O.mxint_quantize(x, **kw, decompose=True)
        cblk, restore = O._blocks(codes.float(), list(kw["block_size"]), kw["skip_first_dim"])
        rebuilt = restore(cblk * torch.pow(2.0, (exps.float() - (kw["width"] - 1)))[..., None])
        ref = torch.where(x.abs() <= 1e-8, torch.zeros_like(y), y)
        assert torch.equal(rebuilt, ref), name
        assert int(codes.abs().max()) <= 2 ** (kw["width"] - 1) - 1
        eb = 2 ** (kw["exponent_width"] - 1) - 1 if kw["exponent_bias"] is None else kw["exponent_bias"]
        xb, _ = O._blocks(x, list(kw["block_size"]), kw["skip_first_dim"])
        nz = xb.abs().amax(dim=-1) != 0
        assert int(exps[nz].min()) >= -eb and int(exps[nz].max()) <= 2 ** kw["exponent_width"] - 1 - eb, name

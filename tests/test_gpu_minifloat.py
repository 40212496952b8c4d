"""The reference's `minifloat` quantizer on the HIP path: the standalone quantizer, bias / weight images, the bf16 activation image,
the Linear forwards with minifloat in every role, full-size token counts, graphs, packed checkpoints, the attention products, and the
C ABI's refusals.  Checked against the reference's vectors (tests/golden/minifloat.npz, forward_minifloat.npz) and the test-local
statement tests/_minifloat.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _minifloat as MF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "minifloat.npz"))
KEYS = sorted({k.split("/")[0] for k in GOLD.files})
FWD = np.load(os.path.join(HERE, "golden", "forward_minifloat.npz"))
with open(os.path.join(HERE, "golden", "forward_minifloat.json")) as fh:
    FWD_CFG = json.load(fh)
W4 = [(4, 2, 1), (4, 2, 7), (4, 1, None), (4, 3, None), (3, 1, None), (2, 1, None)]


@pytest.fixture(scope="module")
def lq():
    import lqer_amd

    return lqer_amd


def mf(w, ew, eb=None):
    return dict(name="minifloat", width=w, exponent_width=ew, exponent_bias=eb)


def fmt_of(key):
    w, ew, b = (int(v) for v in GOLD[f"{key}/fmt"])
    return w, ew, b


def same_bits(a, b):
    return torch.equal(a.float().cpu().view(torch.int32), b.float().cpu().view(torch.int32))


@pytest.mark.parametrize("key", KEYS)
def test_quantizer_vectors(lq, key):
    from lqer_amd import ops

    w, ew, b = fmt_of(key)
    fmt = ops.make_qfmt(mf(w, ew, b), "x")
    x = torch.from_numpy(GOLD[f"{key}/x"])
    out = ops.quantize_mxint(x.to(DEV), fmt, want=("deq", "codes"))
    assert same_bits(out["deq"], torch.from_numpy(GOLD[f"{key}/y"]))
    # codes: sign << (w-1) | magnitude code, whose value table is MF.values
    codes = out["codes"].cpu().to(torch.int32) & 0xFF
    vals = MF.values(w, ew, b)
    dec = vals[codes & ((1 << (w - 1)) - 1)] * torch.where((codes >> (w - 1)) & 1 == 1, -1.0, 1.0)
    y = torch.from_numpy(GOLD[f"{key}/y"])
    assert torch.equal(dec, torch.where(x.abs() <= 1e-8, torch.zeros_like(y), y))
    # fp16 and bf16 tensors: upcast, then the fp32 quantizer
    x16 = torch.from_numpy(GOLD[f"{key}/x16"])
    assert same_bits(ops.quantize_mxint(x16.to(DEV), fmt, want=("deq",))["deq"], torch.from_numpy(GOLD[f"{key}/y16_fp32"]))
    xb = x.clamp(-1e38, 1e38).bfloat16()
    assert same_bits(ops.quantize_mxint(xb.to(DEV), fmt, want=("deq",))["deq"], MF.minifloat(xb.float(), w, ew, b))


def test_bias_pack(lq):
    from lqer_amd import ops

    torch.manual_seed(3)
    b = torch.randn(300) * 3
    b[5] = 5e-9
    for f in ((8, 4, 7), (8, 5, 15), (6, 2, None)):
        got = ops.pack_bias(b.to(DEV), ops.make_qfmt(mf(*f), "b")).cpu()
        assert same_bits(got[:300], MF.minifloat(b, *f)) and not got[300:].any()


@pytest.mark.parametrize("f", W4)
def test_weight_pack_unpack(lq, f):
    from lqer_amd import ops

    torch.manual_seed(11)
    top = float(MF.values(*f).max())
    W = torch.randn(272, 200) * top / 2
    W[0, :8] = torch.tensor([0.0, 1e-9, -1e-9, top * 4, -top * 4, top, -top, 1e-8])
    fmt = ops.make_qfmt(mf(*f), "w")
    Wd = W.to(DEV)
    packed = ops.pack_weight(Wd, fmt)
    got = ops.unpack_weight(packed, 272, 200, fmt).cpu()
    want = MF.minifloat(W, *f)
    assert torch.equal(got, torch.where(W.abs() <= 1e-8, torch.zeros_like(want), want))
    assert torch.equal(ops.quantize_mxint(Wd, fmt, want=("deq",))["deq"].cpu(), want)


def test_activation_image(lq):
    from lqer_amd import ops

    torch.manual_seed(5)
    x = torch.randn(37, 200) * 50
    x[0, :3] = torch.tensor([1e-9, -3e-9, 1000.0])
    for f in ((8, 4, 7), (8, 5, 15), (6, 3, None)):
        img = ops.quantize_act(x.to(DEV), ops.make_qfmt(mf(*f), "x")).cpu()
        want = MF.minifloat(x, *f)
        want = torch.where(x.abs() <= 1e-8, torch.zeros_like(want), want)
        assert torch.equal(img[:37, :200].float(), want)
        assert not img[:37, 200:].float().any()  # (zero-filled beyond K; rows beyond M are not written)


def _module(lq, name, dtype=torch.float32):
    c = FWD_CFG[name]
    qc, r, has_b = c["q_config"], c["rank"], c["bias"]
    W = torch.from_numpy(FWD[f"{name}/W"])
    N, K = W.shape
    if r:
        mod = lq.LinearFlexibleLqer(K, N, bias=has_b, q_config=qc, l_config={"rank": r})
        sd = {"weight": W, "A": torch.from_numpy(FWD[f"{name}/A"]), "B": torch.from_numpy(FWD[f"{name}/B"])}
    else:
        mod = lq.LinearFlexible(K, N, bias=has_b, q_config=qc)
        sd = {"weight": W}
    if has_b:
        sd["bias"] = torch.from_numpy(FWD[f"{name}/bias"])
    mod.load_state_dict(sd)
    return mod.to(DEV).to(dtype)


@pytest.mark.parametrize("name", sorted(FWD_CFG))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_forward_fixtures(lq, name, dtype):
    mod = _module(lq, name, dtype)
    x = torch.from_numpy(FWD[f"{name}/x"])
    y = mod(x.to(dtype).to(DEV)).float().cpu()
    if dtype == torch.float32:
        ref = torch.from_numpy(FWD[f"{name}/y"])
        if FWD_CFG[name]["q_config"]["w_quantizer"]["name"] == "minifloat" and f"{name}/wq" in FWD.files:  # the minifloat weight in place: the reference's bits
            assert same_bits(mod.weight.detach().cpu(), torch.from_numpy(FWD[f"{name}/wq"]))
        bound = 1e-5
    else:  # fp16 module: the checker on the fp16-rounded operands, fp32 arithmetic
        c = FWD_CFG[name]
        W = torch.from_numpy(FWD[f"{name}/W"]).half().float()
        b = torch.from_numpy(FWD[f"{name}/bias"]).half().float() if c["bias"] else None
        A = torch.from_numpy(FWD[f"{name}/A"]).half().float() if c["rank"] else None
        B = torch.from_numpy(FWD[f"{name}/B"]).half().float() if c["rank"] else None
        ref = MF.linear_forward(x.half().float(), W, b, A, B, c["q_config"])
        bound = 1e-3
    err = float((y - ref).norm() / ref.norm())
    assert err <= bound, err


CFG_C2 = dict(name="flexible_lqer", is_ptq=True, default=False, x_quantizer=mf(8, 4, 7), w_quantizer=mf(4, 2, 7), b_quantizer=mf(8, 4, 7))


@pytest.mark.parametrize("M", [1, 7, 64, 300, 2048])
def test_fullsize(lq, M):
    K = N = 4096
    r = 32
    torch.manual_seed(M)
    x = torch.randn(M, K)
    W = 0.02 * torch.randn(N, K)
    A = torch.randn(K, r) / 64
    B = torch.randn(r, N) / 64
    mod = lq.LinearFlexibleLqer(K, N, bias=False, q_config=CFG_C2, l_config={"rank": r})
    mod.load_state_dict({"weight": W, "A": A, "B": B})
    mod = mod.to(DEV)
    y = mod(x.to(DEV)).cpu()
    ref = MF.linear_forward(x, W, None, A, B, CFG_C2)
    err = float((y - ref).norm() / ref.norm())
    assert err <= 1e-4, err  # (x A summed in another order over K = 4096: an A_out / B_out code may flip at a tie)
    y2 = mod(x.to(DEV)).cpu()
    assert torch.equal(y, y2)  # run to run


def test_graph_capture(lq):
    from lqer_amd.graph import GraphedCallable

    K, N, r, M = 512, 384, 32, 96
    torch.manual_seed(9)
    x = torch.randn(M, K)
    mod = lq.LinearFlexibleLqer(K, N, bias=True, q_config=CFG_C2, l_config={"rank": r})
    mod.load_state_dict({"weight": 0.05 * torch.randn(N, K), "bias": torch.randn(N) * 0.1, "A": torch.randn(K, r) / 16,
                         "B": torch.randn(r, N) / 16})
    mod = mod.to(DEV).half()
    xs = x.half().to(DEV)
    mod(xs)
    gc = GraphedCallable(mod, xs.clone(), warmup=1)
    for scale in (1.0, -0.5, 3.0):
        xn = (x * scale).half().to(DEV)
        ref = mod(xn).clone()
        got = gc(xn).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, ref), scale


def test_packed_checkpoint(lq):
    name = "all_roles"
    mod = _module(lq, name)
    x = torch.from_numpy(FWD[f"{name}/x"]).to(DEV)
    want = mod(x)
    st = {k: v.cpu() for k, v in mod.packed_state().items()}
    c = FWD_CFG[name]
    N, K = FWD[f"{name}/W"].shape
    m2 = lq.LinearFlexibleLqer(K, N, bias=c["bias"], q_config=c["q_config"], l_config={"rank": c["rank"]})
    m2.load_packed_state(st, DEV)
    assert torch.equal(m2.to(DEV)(x), want)
    other = dict(c["q_config"], w_quantizer=mf(4, 2, 6))  # another format: the header check refuses
    m3 = lq.LinearFlexibleLqer(K, N, bias=c["bias"], q_config=other, l_config={"rank": c["rank"]})
    with pytest.raises(RuntimeError):
        m3.load_packed_state(st, DEV)


def test_quantize_model_swap(lq):
    transformers = pytest.importorskip("transformers")
    from lqer_amd.models import quantize_model

    cfg = transformers.LlamaConfig(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4,
                                   num_key_value_heads=4, max_position_embeddings=64)
    torch.manual_seed(0)
    model = transformers.LlamaForCausalLM(cfg).eval()
    quantize_model(model, {"linear": CFG_C2}, {"linear": {"rank": 16}})
    mods = [m for m in model.modules() if isinstance(m, lq.LinearFlexibleLqer)]
    assert len(mods) == 7 and all(m._group is None for m in mods)  # minifloat: every projection runs its own forward
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in mods:
            m.A.copy_(0.02 * torch.randn(m.in_features, 16, generator=g))
            m.B.copy_(0.02 * torch.randn(16, m.out_features, generator=g))
    model = model.to(DEV)
    ids = torch.randint(0, 64, (2, 9))
    x = torch.randn(2, 9, 128, device=DEV)
    q = model.model.layers[0].self_attn.q_proj
    y = q(x).cpu()
    ref = MF.linear_forward(x.cpu(), q.weight.detach().cpu(), None, q.A.detach().cpu(), q.B.detach().cpu(), CFG_C2)
    assert float((y - ref).norm() / ref.norm()) <= 1e-5
    with torch.no_grad():
        out = model(ids.to(DEV)).logits
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("style", ["matmul", "bmm"])
def test_matmul_flexible(lq, style):
    from lqer_amd import functional as FN

    torch.manual_seed(21)
    x = torch.randn(3, 40, 64)
    y = torch.randn(3, 64, 48)
    qc = dict(name="flexible", default=None, x_quantizer=mf(8, 4, 7), w_quantizer=mf(6, 3))
    fn = FN.matmul_flexible if style == "matmul" else FN.bmm_flexible
    got = fn(x.to(DEV), y.to(DEV), qc).cpu()
    ref = torch.matmul(MF.minifloat(x, 8, 4, 7), MF.minifloat(y, 6, 3))
    assert float((got - ref).norm() / ref.norm()) <= 1e-6
    mixed = dict(qc, w_quantizer=dict(name="block_fp", width=8, exponent_width=8, exponent_bias=None, block_size=[1, 16], skip_first_dim=True))
    from oracle import lqer_oracle as O

    got2 = fn(x.to(DEV), y.to(DEV), mixed).cpu()
    ref2 = torch.matmul(MF.minifloat(x, 8, 4, 7), O.get_quantizer(mixed["w_quantizer"])(y))
    assert float((got2 - ref2).norm() / ref2.norm()) <= 1e-6


def test_c_abi_refusals(lq):
    from lqer_amd import _lib

    L = _lib.lib()
    W = torch.randn(32, 64, device=DEV)
    out = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    scr = torch.empty(4096, dtype=torch.int8, device=DEV)
    f6 = _lib.QFmt(_lib.Q_MINIFLOAT, 6, -1, 3, 3)
    rc = L.lqer_pack_weight_mxint(W.data_ptr(), _lib.F32, 32, 64, 64, C.byref(f6), out.data_ptr(), scr.data_ptr(), None)
    assert rc == -2 and b"minifloat" in L.lqer_last_error()
    bad = _lib.QFmt(_lib.Q_MINIFLOAT, 8, -1, 8, 7)  # exp_width 8 leaves no sign bit
    deq = torch.empty(32, 64, device=DEV)
    rc = L.lqer_quantize_mxint(W.data_ptr(), _lib.F32, 32, 64, 64, C.byref(bad), deq.data_ptr(), None, None, None)
    assert rc == -2 and b"exponent_width" in L.lqer_last_error()


def _bfp(width, block, skip=True):
    return dict(name="block_fp", width=width, exponent_width=8, exponent_bias=None, block_size=block, skip_first_dim=skip)


# the GEMM instantiations of each (weight kind, B_out kind) pair that no fixture reaches, and the pass-through fp16 activations with a
# minifloat B_out (the bf16 limb route: the fp16 main loop has no minifloat B_out)
EXTRA = {
    "intw_mfbout": dict(CFG_C2, x_quantizer=_bfp(8, [1, 16]), w_quantizer=dict(name="integer", width=4, frac_width=7), b_quantizer=_bfp(8, [-1], False),
                        A_out_quantizer=_bfp(8, [1, 16]), B_out_quantizer=mf(8, 4, 10)),
    "mfw_passbout": dict(CFG_C2, B_out_quantizer=dict(name="passthrough")),
    "mfw_bfp32bout": dict(CFG_C2, B_out_quantizer=_bfp(8, [1, 32])),
    "mfw_intbout": dict(CFG_C2, B_out_quantizer=dict(name="integer", width=8, frac_width=6)),
    "a16_mfbout": dict(CFG_C2, x_quantizer=dict(name="passthrough"), w_quantizer=_bfp(4, [1, 16], False), b_quantizer=dict(name="passthrough"),
                       B_out_quantizer=mf(8, 4, 10)),
}


@pytest.mark.parametrize("name", sorted(EXTRA))
@pytest.mark.parametrize("M", [5, 300])
def test_forward_weight_bout_pairs(lq, name, M):
    qc = EXTRA[name]
    K, N, r = 192, 288, 32
    torch.manual_seed(M + len(name))
    x = torch.randn(M, K)
    W = 0.02 * torch.randn(N, K)
    bias = 0.01 * torch.randn(N)
    A, B = torch.randn(K, r) / 16, torch.randn(r, N) / 16
    dtype = torch.float16 if name.startswith("a16") else torch.float32
    mod = lq.LinearFlexibleLqer(K, N, bias=True, q_config=qc, l_config={"rank": r})
    mod.load_state_dict({"weight": W, "bias": bias, "A": A, "B": B})
    mod = mod.to(DEV).to(dtype)
    y = mod(x.to(dtype).to(DEV)).float().cpu()
    assert not mod._x_f16 and not mod._x_i8
    cast = (lambda t: t.half().float()) if dtype == torch.float16 else (lambda t: t)
    ref = MF.linear_forward(cast(x), cast(W), cast(bias), cast(A), cast(B), qc)
    err = float((y - ref).norm() / ref.norm())
    assert err <= (1e-3 if dtype == torch.float16 else 1e-4), err
    assert torch.equal(mod(x.to(dtype).to(DEV)).float().cpu(), y)


@pytest.mark.parametrize("name", [n for n in sorted(FWD_CFG) if FWD_CFG[n]["rank"]])
def test_fixture_images(lq, name):
    """The activation image bit for bit the reference's x_quantizer (|x| <= 1e-8 flushed), and xAq inside the summation-order
    envelope of the exact sum xq A (tests/_envelope.py for block_fp A_out, MF.envelope_bad for minifloat)."""
    import math

    from _envelope import envelope_check
    from lqer_amd import _lib

    mod = _module(lq, name)
    x = torch.from_numpy(FWD[f"{name}/x"])
    mod(x.to(DEV))  # (packs the images)
    K = mod.in_features
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    L = _lib.lib()
    desc = mod._desc()
    p = mod._packed
    rp = L.lqer_padded_r(mod.rank)
    xq = torch.zeros(L.lqer_act_image_bytes(C.byref(desc), M) // 2, dtype=torch.bfloat16, device=DEV)
    xaq = torch.zeros(L.lqer_padded_m(M), rp, dtype=torch.bfloat16, device=DEV)
    nscr = L.lqer_lowrank_xa_scratch_bytes(C.byref(desc), M)
    scr = torch.empty(max(nscr, 16), dtype=torch.uint8, device=DEV)
    xd = x2.contiguous().to(DEV)
    _lib.check(L.lqer_quantize_act_xa(C.byref(desc), xd.data_ptr(), _lib.F32, M, K, p["a_t"].data_ptr(), int(p["a_limbs"]), xq.data_ptr(),
                                      xaq.data_ptr(), scr.data_ptr(), nscr, None), "quantize_act_xa")
    torch.cuda.synchronize()
    img = xq[: L.lqer_padded_m(M) * L.lqer_padded_k(K)].view(L.lqer_padded_m(M), L.lqer_padded_k(K))[:M, :K].float().cpu()
    want = torch.from_numpy(FWD[f"{name}/xq"]).reshape(-1, K)
    assert torch.equal(img, torch.where(x2.abs() <= 1e-8, torch.zeros_like(want), want))
    s64 = img.double().numpy() @ torch.from_numpy(FWD[f"{name}/A"]).double().numpy()
    got = xaq[:M, : mod.rank].float().cpu().numpy()
    D = max(16.0, math.sqrt(K))
    qa = FWD_CFG[name]["q_config"].get("A_out_quantizer", FWD_CFG[name]["q_config"]["x_quantizer"])
    if qa["name"] == "minifloat":
        assert MF.envelope_bad(s64, got, qa["width"], qa["exponent_width"], qa.get("exponent_bias"), D) == 0
    else:
        assert envelope_check(s64, got, 16, qa["width"] - 1, D) == 0

"""The compact image of 2- / 3-bit block_fp weights on the GPU (include/lqer_hip.h "compact weight image"): the device conversions
against their host twins, the decode-size kernels reading the compact image (bit-equal to the standard image's forward, and within
tests/test_gpu_decode1.py's tolerances of the oracle), the widen route of every other kernel, shared inputs, guard zones around the
compact image and the workspace, and the module / packed-checkpoint surface.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _narrow_ref as R  # noqa: E402
from oracle import lqer_oracle as O  # noqa: E402  (the checker)

DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3, torch.float32: 1e-5}  # tests/test_gpu_decode1.py
FORMATS = [(2, 16), (2, 32), (3, 32), (3, 16), (3, 128), (2, -1), (3, 48)]  # (width, block)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lqer_amd import ops as _ops

    return _ops


def _cfgs():
    from bench import MXINT_Q, W3A16_Q, _bfp

    return {
        "w2b16": dict(MXINT_Q, w_quantizer=_bfp(2, [1, 16], False)),
        "w3b16": dict(MXINT_Q, w_quantizer=_bfp(3, [1, 16], False)),
        "w3a16": W3A16_Q,
        "w2row": dict(MXINT_Q, w_quantizer=_bfp(2, [1, -1], False), B_out_quantizer=dict(name="passthrough")),
        "w2b16_boutrow": dict(MXINT_Q, w_quantizer=_bfp(2, [1, 16], False), B_out_quantizer=_bfp(8, [1, -1], True)),
    }


def _pair(K, N, r, bias, cfg, dtype, seed=5, M=64):
    """The same operands in two modules: weight_image "standard" and "narrow"."""
    import lqer_amd
    from bench import UNQUANTIZED_AB, make_case

    case = make_case(M, K, N, r, seed=seed, bias=bias, quantize_ab=not any(cfg is c for c in UNQUANTIZED_AB))
    x, W, A, B = case[:4]
    mods = []
    for image in ("standard", "narrow"):
        mod = lqer_amd.LinearFlexibleLqer(K, N, bias=bias, q_config=cfg, l_config={"rank": r})
        sd = {"weight": W, "A": A, "B": B}
        if bias:
            sd["bias"] = case[4]
        mod.load_state_dict(sd)
        mod.weight_image = image
        mods.append(mod.to(DEV).to(dtype))
    return mods[0], mods[1], x, W, A, B, (case[4] if bias else None)


def _ref(x, W, b, A, B, cfg, dtype):
    h = (lambda t: None if t is None else t.to(dtype).float())
    return O.lqer_linear_forward(h(x), h(W), h(b), h(A), h(B), cfg)


def _route(mod, xd, ops):
    """What lqer_weight_narrow_route says about the call mod(xd) makes."""
    from lqer_amd import _lib

    p = mod._packed
    x2 = xd.reshape(-1, xd.shape[-1])
    M = x2.shape[0]
    desc = mod._desc()
    return _lib.lib().lqer_weight_narrow_route(C.byref(desc), M, ops.dtype_code(x2), x2.stride(0) if M > 1 else x2.shape[1],
                                               int(p.get("a_limbs", 0)), int(p.get("b_limbs", 0)))


# ---- conversions ------------------------------------------------------------------------------------------------------------------

def _packed_image(ops, width, block, N, K, rows=1, seed=3):
    from bench import _bfp

    g = torch.Generator().manual_seed(seed)
    W = (0.02 * torch.randn(N, K, generator=g)).to(DEV)
    W[1, 32:64] = 0.0  # an all-zero block
    fmt = ops.make_qfmt(_bfp(width, [rows, block], False), "w")
    return ops.pack_weight(W, fmt), fmt


@pytest.mark.parametrize("width,block", FORMATS)
def test_device_conversions_match_the_host_and_round_trip(ops, width, block):
    from lqer_amd import _lib

    N, K = 48, 200
    img, fmt = _packed_image(ops, width, block, N, K)
    nar = ops.weight_narrow(img, N, K, fmt)
    assert nar.numel() == ops.weight_narrow_bytes(N, K, fmt)
    back = ops.weight_widen(nar, N, K, fmt)
    torch.cuda.synchronize()
    assert torch.equal(back, img)
    host_in = np.ascontiguousarray(img.cpu().numpy())
    host_out = np.zeros(nar.numel(), dtype=np.uint8)
    assert host_in.ctypes.data % 16 == 0 and host_out.ctypes.data % 16 == 0
    _lib.check(_lib.lib().lqer_weight_narrow_host(host_in.ctypes.data, N, K, C.byref(fmt), host_out.ctypes.data), "lqer_weight_narrow_host")
    assert np.array_equal(nar.cpu().numpy(), host_out)


def test_two_d_tiles_round_trip(ops):
    N, K = 48, 200
    img, fmt = _packed_image(ops, 3, 32, N, K, rows=4)
    assert int(getattr(fmt, "block_rows", 1)) == 4
    nar = ops.weight_narrow(img, N, K, fmt)
    assert torch.equal(ops.weight_widen(nar, N, K, fmt), img)
    assert nar.numel() == (256 // 16) * (256 // 64) * 416


# ---- the decode-size kernels read the compact image -------------------------------------------------------------------------------

DIRECT = [("w2b16", torch.float16), ("w2b16", torch.bfloat16), ("w2b16", torch.float32),
          ("w3b16", torch.float16), ("w3b16", torch.bfloat16), ("w3b16", torch.float32),
          ("w3a16", torch.float16), ("w2row", torch.float16)]
SHAPES = {"large": (4688, 272, 32, True, (1, 8, 9, 33, 64, -7)),  # (-7: 7 tokens with a row stride that is not 16-byte aligned)
          "small": (128, 48, 16, False, (1, 5))}


@pytest.mark.parametrize("shape", ["large", "small"])
@pytest.mark.parametrize("name,dtype", DIRECT)
def test_decode_kernels_read_the_compact_image(ops, name, dtype, shape):
    from lqer_amd import _lib

    cfg = _cfgs()[name]
    K, N, r, bias, Ms = SHAPES[shape]
    std, nar, x, W, A, B, b = _pair(K, N, r, bias, cfg, dtype)
    ref = _ref(x, W, b, A, B, cfg, dtype)  # every row once; a token's row does not depend on the others
    mxint = name != "w3a16"
    for M in Ms:
        if M < 0:
            M = -M
            wide = torch.zeros(M, K + 1, dtype=dtype, device=DEV)
            wide[:, :K] = x[:M].to(dtype).to(DEV)
            xd = wide[:, :K]
            assert (xd.stride(0) * xd.element_size()) % 16 != 0
            want_route = _lib.NARROW_DIRECT
        else:
            xd = x[:M].to(dtype).to(DEV)
            want_route = _lib.NARROW_DIRECT_ONE_LAUNCH if (mxint and M <= 8) else _lib.NARROW_DIRECT
        y_std, y_nar = std(xd), nar(xd)
        torch.cuda.synchronize()
        assert nar._packed["w"].numel() == ops.weight_narrow_bytes(N, K, nar._fmt["w"])
        assert _route(nar, xd, ops) == want_route, (M, _route(nar, xd, ops))
        assert torch.equal(y_nar, y_std), (name, dtype, shape, M)
        err = float((y_nar.float().cpu() - ref[:M]).norm() / ref[:M].norm())
        print(f"narrow {name} {dtype} {shape} M={M}: rel-L2 vs oracle {err:.3e}")
        assert err <= TOL[dtype], (M, err)


def test_one_launch_fallback_gives_the_same_bits(ops):
    from lqer_amd import _lib

    K, N, r, bias, _ = SHAPES["large"]
    std, nar, x, *_ = _pair(K, N, r, bias, _cfgs()["w3b16"], torch.float16)
    xd = x[:8].half().to(DEV)
    y = nar(xd)
    assert _route(nar, xd, ops) == _lib.NARROW_DIRECT_ONE_LAUNCH
    nar.tuning = _lib.TUNE_DECODE_NO_POLL  # every consumer workgroup computes the partial tiles of x A itself
    y_fb = nar(xd)
    assert torch.equal(y_fb, y) and torch.equal(y, std(xd))


# ---- every other route widens first ------------------------------------------------------------------------------------------------

def test_larger_token_counts_widen_into_the_workspace(ops):
    from lqer_amd import _lib

    K, N, r, bias, _ = SHAPES["large"]
    std, nar, x, *_ = _pair(K, N, r, bias, _cfgs()["w2b16"], torch.float16, M=300)
    for M in (65, 300):
        xd = x[:M].half().to(DEV)
        y = nar(xd)
        assert _route(nar, xd, ops) == _lib.NARROW_WIDEN
        assert torch.equal(y, std(xd)), M


def test_decode_size_on_the_tile_kernel_widens(ops):
    from lqer_amd import _lib

    K, N, r, bias, _ = SHAPES["large"]
    std, nar, x, *_ = _pair(K, N, r, bias, _cfgs()["w2b16_boutrow"], torch.float16)
    xd = x[:3].half().to(DEV)
    y = nar(xd)
    assert _route(nar, xd, ops) == _lib.NARROW_WIDEN
    assert _lib.lib().lqer_gemm_route(C.byref(nar._desc()), 3, _lib.F16) == _lib.ROUTE_TILE128
    assert torch.equal(y, std(xd))


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------

def test_shared_activation_with_narrow_members(ops):
    import lqer_amd
    from bench import make_case
    from lqer_amd.linear import SharedActivation

    cfg = _cfgs()["w2b16"]
    K, r = 256, 16
    mods, x = [], None
    for i, N in enumerate((48, 48, 96)):
        case = make_case(70, K, N, r, seed=40 + i)
        x = case[0] if x is None else x
        m = lqer_amd.LinearFlexibleLqer(K, N, bias=False, q_config=cfg, l_config={"rank": r})
        m.load_state_dict({"weight": case[1], "A": case[2], "B": case[3]})
        m.weight_image = "narrow"
        mods.append(m.to(DEV).half())
    for M in (4, 70):
        xd = x[:M].half().to(DEV)
        alone = [m(xd).clone() for m in mods]
        grp = SharedActivation(mods)
        assert grp.enabled
        got = [m(xd) for m in mods]
        torch.cuda.synchronize()
        assert grp._dplans.get((M, ops.dtype_code(xd))) is None  # a group launch takes standard images only
        assert grp._cur is not None                               # ... the members ran behind the shared activation
        for i, (a, g_) in enumerate(zip(alone, got)):
            assert torch.equal(a, g_), (M, i)
        for m in mods:
            m._group = None


# ---- guard zones ----------------------------------------------------------------------------------------------------------------------

def test_guard_zones_around_the_compact_image_and_the_workspace(ops):
    from _guard import guarded
    from lqer_amd import _lib

    L = _lib.lib()
    K, N, r, bias, _ = SHAPES["large"]
    std, nar, x, *_ = _pair(K, N, r, bias, _cfgs()["w3b16"], torch.float16, M=70)
    xd70 = x[:70].half().to(DEV)
    y_ref = {5: std(xd70[:5]).clone(), 70: std(xd70).clone()}
    nar.pack()
    fmt, p = nar._fmt["w"], nar._packed
    nb = ops.weight_narrow_bytes(N, K, fmt)
    std_img = std._packed["w"].reshape(-1).view(torch.uint8)
    # conversions: the compact image and the standard image are exactly their sizes
    g_std = guarded(std_img.numel(), name="standard image").load(std_img)
    g_nar = guarded(nb, name="compact image")
    _lib.check(L.lqer_weight_narrow(g_std.ptr, N, K, C.byref(fmt), g_nar.ptr, None), "narrow")
    torch.cuda.synchronize()
    g_nar.check(), g_std.unchanged()
    assert torch.equal(g_nar.payload, p["w"].reshape(-1).view(torch.uint8))
    g_nar.snapshot = g_nar.arena.clone()
    g_back = guarded(std_img.numel(), fill=0xFF, name="widened image")
    _lib.check(L.lqer_weight_widen(g_nar.ptr, N, K, C.byref(fmt), g_back.ptr, None), "widen")
    torch.cuda.synchronize()
    g_back.check(), g_nar.unchanged()
    assert torch.equal(g_back.payload, std_img)
    # forwards: one direct call (M = 5, one launch) and one widen call (M = 70) with the workspace exactly as reported
    for M, want in ((5, _lib.NARROW_DIRECT_ONE_LAUNCH), (70, _lib.NARROW_WIDEN)):
        xd = xd70[:M].contiguous()
        desc = nar._desc()
        dt = ops.dtype_code(xd)
        assert _route(nar, xd, ops) == want
        ws_bytes = L.lqer_linear_forward_narrow_workspace_bytes(C.byref(desc), M)
        g_ws = guarded(ws_bytes, fill=0xFF, name=f"workspace M={M}")
        g_y = guarded(M * N * 2, fill=0xFF, name=f"y M={M}")
        a_t, a_limbs = nar._side_image(M, desc, dt)
        _lib.check(L.lqer_linear_forward_narrow(C.byref(desc), xd.data_ptr(), dt, M, K, g_nar.ptr, a_t, ops._ptr(p.get("b_t")), a_limbs,
                                                p.get("b_limbs", 0), ops._ptr(p.get("bias")), g_y.ptr, N, g_ws.ptr, ws_bytes, None),
                   "lqer_linear_forward_narrow")
        torch.cuda.synchronize()
        g_ws.check(), g_y.check(), g_nar.unchanged()
        assert torch.equal(g_y.view(torch.float16).reshape(M, N), y_ref[M])
        # one byte less is refused before anything is launched
        if ws_bytes:
            assert L.lqer_linear_forward_narrow(C.byref(desc), xd.data_ptr(), dt, M, K, g_nar.ptr, a_t, ops._ptr(p.get("b_t")), a_limbs,
                                                p.get("b_limbs", 0), ops._ptr(p.get("bias")), g_y.ptr, N, g_ws.ptr, ws_bytes - 1, None) == -4


# ---- module and checkpoint ------------------------------------------------------------------------------------------------------------

def test_narrow_module_holds_only_the_compact_image(ops):
    K, N, r = 128, 48, 16
    std, nar, x, *_ = _pair(K, N, r, False, _cfgs()["w3b16"], torch.float16)
    nar.pack(), std.pack()
    nb = ops.weight_narrow_bytes(N, K, nar._fmt["w"])
    assert nb == (256 // 16) * (128 // 64) * 448
    assert nar._packed["w"].numel() == nb and nar._w_single.numel() == nb
    assert std._packed["w"].numel() == (256 // 16) * (128 // 64) * 576
    assert not any(torch.is_tensor(v) and v.numel() * v.element_size() == std._packed["w"].numel() for v in nar._packed.values())
    assert "weight_image=narrow" in repr(nar) and "weight_image" not in repr(std)
    assert torch.equal(nar.weight, std.weight)  # the dense parameter still receives w_quantizer(W)
    # the attribute after the first forward: the derived images are dropped and rebuilt in the other kind, the weight quantized once
    xd = x[:2].half().to(DEV)
    y = nar(xd)
    nar.weight_image = "standard"
    assert nar._packed is None
    assert torch.equal(nar(xd), y) and nar._packed["w"].numel() == std._packed["w"].numel()
    nar.weight_image = "narrow"
    assert torch.equal(nar(xd), y) and nar._packed["w"].numel() == nb


@pytest.mark.parametrize("src,dst", [("narrow", "narrow"), ("narrow", "standard"), ("standard", "narrow")])
def test_packed_state_round_trips_between_image_kinds(ops, src, dst):
    import lqer_amd

    K, N, r = 128, 48, 16
    cfg = _cfgs()["w2b16"]
    std, nar, x, *_ = _pair(K, N, r, True, cfg, torch.float16)
    xd = x[:2].half().to(DEV)
    mod = nar if src == "narrow" else std
    y = mod(xd)
    state = mod.packed_state()
    assert ("w_narrow" in state) == (src == "narrow") and ("w" in state) == (src == "standard")
    new = lqer_amd.LinearFlexibleLqer(K, N, bias=True, q_config=cfg, l_config={"rank": r}).to(DEV).half()
    new.weight_image = dst
    new.load_packed_state({k: v.cpu() for k, v in state.items()}, DEV)
    want = ops.weight_narrow_bytes(N, K, new._fmt["w"]) if dst == "narrow" else (256 // 16) * (128 // 64) * 576
    assert new._packed["w"].numel() == want
    assert torch.equal(new(xd), y)


def test_width_4_narrow_module_raises_at_pack(ops):
    import lqer_amd
    from bench import MXINT_Q, make_case

    x, W, A, B = make_case(2, 128, 48, 16, seed=1)
    mod = lqer_amd.LinearFlexibleLqer(128, 48, bias=False, q_config=MXINT_Q, l_config={"rank": 16})
    mod.load_state_dict({"weight": W, "A": A, "B": B})
    mod.weight_image = "narrow"
    mod = mod.to(DEV).half()
    with pytest.raises(NotImplementedError, match="width 2 or 3"):
        mod.pack()
    with pytest.raises(ValueError):
        mod.weight_image = "compact"

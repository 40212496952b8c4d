"""WHERE the kernels write: every C-ABI call between guard zones (tests/_guard.py).  Every buffer a call writes is a guarded payload of
exactly its documented size, workspace / scratch sizes are exactly the reported values, row strides are padded (wide stores legal, then
forced onto the element path), token counts sit one row above and below the tile boundaries.  Per call: (a) every guard, every gap
between rows and every read-only input is bit-unchanged, (b) the output equals, bit for bit, the module's own result for the same
input (those values are pinned to the oracle by the rest of the suite: equality here proves that every element was written and that
nothing depends on strides or placement), (c) the same call over arenas filled with 0xFF (NaN in every float type) gives the same
bits - the workspace and the never-written rows M..Mp-1 of the images included -, (d) a workspace one byte short is refused on the host.
No value tolerance anywhere: every comparison is bit equality.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import ctypes as C
import os
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _footprint_cases as FC  # noqa: E402
from _guard import guarded, rows_bytes  # noqa: E402

DEV = "cuda:0"
FILLS = (1, 0xFF)  # a seeded pseudo-random pattern, then 0xFF


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import lqer_amd

    return lqer_amd


def _esz(dt):
    return 4 if dt == torch.float32 else 2


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.numel() == b.numel(), what
    d = (a != b).nonzero()
    assert d.numel() == 0, f"{what}: {d.numel()} byte(s) differ, first at byte {int(d[0])}, last at byte {int(d[-1])}"


def _operands(case):
    """(x, W, A, B, bias) on the CPU in fp32 from one seed per case; A / B on the 8-bit MXINT grid unless the configuration keeps them
    unquantized (one bf16 limb: what the decode kernels and the a_limbs = -2 image need)."""
    from bench import _snap_mxint8_dim0

    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    x = torch.randn(case.M, case.K, generator=g)
    x[:, 7] *= 30.0
    W = 0.02 * torch.randn(case.N, case.K, generator=g)
    A = B = b = None
    if case.r > 0:
        A, B = 0.01 * torch.randn(case.K, case.r, generator=g), 0.01 * torch.randn(case.r, case.N, generator=g)
        if case.cfg not in FC.UNQUANTIZED_AB:
            A, B = _snap_mxint8_dim0(A), _snap_mxint8_dim0(B)
    if case.bias:
        b = 0.01 * torch.randn(case.N, generator=g)
    return x, W, A, B, b


def _module(case):
    x, W, A, B, b = _operands(case)
    mod = FC.make_module(case)
    sd = {"weight": W}
    if case.r > 0:
        sd.update(A=A, B=B)
    if b is not None:
        sd["bias"] = b
    mod.load_state_dict(sd)
    dt = FC.DTYPES[case.dtype]
    mod = mod.to(DEV).to(dt)
    for k, v in case.flags.items():
        setattr(mod, k, v)
    mod.tuning = FC.tuning_bits(case)
    mod.pack()
    kind = "i8" if mod._x_i8 else ("f16" if mod._x_f16 else ("pass" if mod._fmt["x"].kind == 0 else "mx"))
    assert kind == case.x_kind, f"{case.id}: the packing chose x format '{kind}', the case table (and its CPU route check) says '{case.x_kind}'"
    return mod, x.to(dt).to(DEV)


def _side_tensor(mod, M, desc, dtc):
    """The A^T image tensor and limb code a forward of M tokens is handed - LinearFlexible._side_image, with the tensor."""
    from lqer_amd import _lib

    p = mod._packed
    L = _lib.lib()
    if mod._x_i8 and "a_t_f16" in p and L.lqer_gemm_route(C.byref(desc), M, dtc) == _lib.ROUTE_I8:
        t, al = p["a_t_f16"], -1
    elif "a_t_b16" in p and M > 64 and not mod._x_i8:
        t, al = p["a_t_b16"], -2
    else:
        t, al = p.get("a_t"), p.get("a_limbs", 0)
    assert ((None if t is None else t.data_ptr()), al) == tuple(mod._side_image(M, desc, dtc))
    return t, al


def _wrap_input(t, name, fill, align=256):
    if t is None:
        return None
    nbytes = t.numel() * t.element_size()
    return guarded(nbytes, align=align, fill=fill, name=name).load(t)


def _forward_inputs(mod, M, desc, dtc, fill):
    """The packed operands of a forward as guarded read-only inputs of exactly their documented sizes."""
    from lqer_amd import _lib

    L = _lib.lib()
    p = mod._packed
    sz = _lib.LinearSizes()
    assert L.lqer_linear_sizes(C.byref(desc), M, C.byref(sz)) == 0, L.lqer_last_error()
    a_t, a_limbs = _side_tensor(mod, M, desc, dtc)
    K, r = mod.in_features, mod.rank
    assert p["w"].numel() * p["w"].element_size() == sz.w_packed
    if a_t is not None:
        doc = {-1: L.lqer_a_f16_image_bytes(K, r), -2: L.lqer_a_b16_image_bytes(K, r)}.get(
            a_limbs, L.lqer_a_f16_image_bytes(K, r) if mod._x_f16 else sz.a_t)
        assert a_t.numel() * a_t.element_size() == doc, (a_limbs, a_t.numel() * a_t.element_size(), doc)
        assert p["b_t"].numel() * p["b_t"].element_size() == sz.b_t
    if p.get("bias") is not None:
        assert p["bias"].numel() * 4 == sz.bias_q
    ins = {"w_packed": _wrap_input(p["w"], "w_packed", fill), "a_t": _wrap_input(a_t, "a_t", fill),
           "b_t": _wrap_input(p.get("b_t"), "b_t", fill), "bias_q": _wrap_input(p.get("bias"), "bias_q", fill)}
    return ins, a_limbs, p.get("b_limbs", 0), sz


def _ptr(g):
    return None if g is None else g.ptr


def _check_all(outs, ins):
    torch.cuda.synchronize()
    for g in outs:
        g.check()
    for g in ins:
        if g is not None:
            g.unchanged()


@pytest.mark.parametrize("case", FC.CASES, ids=[c.id for c in FC.CASES])
def test_forward_stays_inside_its_buffers(lq, case):
    from lqer_amd import _lib, ops

    L = _lib.lib()
    mod, xd = _module(case)
    dt = xd.dtype
    dtc = ops.dtype_code(xd)
    M, K, N, es = case.M, case.K, case.N, _esz(dt)
    ldx, ldy = K + case.ldx_pad, N + case.ldy_pad
    desc = mod._desc()
    base = mod(xd).clone()  # the module's own forward: dense x, dense y, the grow-only workspace pool
    assert base.shape == (M, N)
    got = {}
    for fill in FILLS:
        ins, a_limbs, b_limbs, sz = _forward_inputs(mod, M, desc, dtc, fill)
        x = guarded(rows_bytes(M, K, ldx, es), row_pitch_bytes=ldx * es, fill=fill, name="x").load_rows(xd, ldx)
        y = guarded(rows_bytes(M, N, ldy, es), row_pitch_bytes=ldy * es, fill=fill, name="y")
        ws = guarded(sz.workspace, fill=fill, name="workspace")
        args = lambda nws: (C.byref(desc), x.ptr, dtc, M, ldx, ins["w_packed"].ptr, _ptr(ins["a_t"]), _ptr(ins["b_t"]), a_limbs, b_limbs,
                            _ptr(ins["bias_q"]), y.ptr, ldy, ws.ptr, nws, None)
        # (d) one byte short: refused on the host, nothing launched
        assert L.lqer_linear_forward(*args(sz.workspace - 1)) == -4, L.lqer_last_error()
        torch.cuda.synchronize()
        y.unchanged(), ws.unchanged()
        rc = L.lqer_linear_forward(*args(sz.workspace))
        assert rc == 0, L.lqer_last_error()
        _check_all([y, ws], [x] + list(ins.values()))          # (a) guards and inputs
        y.gaps_unchanged(M, N, ldy, dt)                           # (a) the gaps between the rows of y
        got[fill] = y.rows_view(M, N, ldy, dt).clone()
        _same_bits(got[fill], base, f"{case.id}: y (fill {fill:#x}) against the module's forward")   # (b), (c)
    _same_bits(got[FILLS[0]], got[FILLS[1]], f"{case.id}: y over a random fill against y over 0xFF")


# ---- group launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns,K,r,M,dtype,ldy_pad,ldx_pad", [((48, 1000), 128, 16, 1, torch.float16, 8, 0),
                                                            ((256, 48, 1000), 208, 20, 5, torch.bfloat16, 3, 8),   # (the one-launch kernel: K a multiple of 16)
                                                            ((1000, 48), 128, 32, 8, torch.float32, 3, 4)])
def test_group_forward_stays_inside_its_buffers(lq, Ns, K, r, M, dtype, ldy_pad, ldx_pad):
    """lqer_linear_forward_group with 2 and 3 members on a workspace of exactly lqer_group_workspace_bytes: per member the bits of its
    own forward, every member's y between guards with a padded stride."""
    from bench import MXINT_Q, _snap_mxint8_dim0
    from lqer_amd import _lib, ops
    from lqer_amd.linear import SharedActivation

    L = _lib.lib()
    g = torch.Generator().manual_seed(len(Ns) * 1000 + K)
    x = torch.randn(M, K, generator=g)
    mods = []
    for i, N in enumerate(Ns):
        m = lq.LinearFlexibleLqer(K, N, bias=(i == 1), q_config=MXINT_Q, l_config={"rank": r})
        sd = {"weight": 0.02 * torch.randn(N, K, generator=g), "A": _snap_mxint8_dim0(0.01 * torch.randn(K, r, generator=g)),
              "B": _snap_mxint8_dim0(0.01 * torch.randn(r, N, generator=g))}
        if i == 1:
            sd["bias"] = 0.01 * torch.randn(N, generator=g)
        m.load_state_dict(sd)
        mods.append(m.to(DEV).to(dtype))
    xd = x.to(dtype).to(DEV)
    alone = [m(xd).clone() for m in mods]
    grp = SharedActivation(mods)
    assert grp.enabled
    grp._pack_cat(torch.device(DEV))
    for m in mods:
        m._group = None
    assert grp._cat["a_limbs"] == 1
    es, dtc = _esz(dtype), ops.dtype_code(xd)
    ldx = K + ldx_pad
    nws = L.lqer_group_workspace_bytes(K, grp._cat["rp_total"])
    descs = [m._desc(plain=True) for m in mods]
    outs = {}
    for fill in FILLS:
        xg = guarded(rows_bytes(M, K, ldx, es), row_pitch_bytes=ldx * es, fill=fill, name="x").load_rows(xd, ldx)
        a_cat = _wrap_input(grp._cat["a_t"], "a_t_cat", fill)
        ws = guarded(nws, fill=fill, align=16, name="group workspace")  # (the contract: 16-byte aligned)
        tab = (_lib.GroupMember * len(mods))()
        ys, ins = [], []
        for i, (m, d) in enumerate(zip(mods, descs)):
            p = m._packed
            ldy = m.out_features + ldy_pad
            yg = guarded(rows_bytes(M, m.out_features, ldy, es), row_pitch_bytes=ldy * es, fill=fill, name=f"y[{i}]")
            w, bt, bq = _wrap_input(p["w"], f"w_packed[{i}]", fill), _wrap_input(p["b_t"], f"b_t[{i}]", fill), _wrap_input(p.get("bias"), f"bias_q[{i}]", fill)
            tab[i].desc, tab[i].w_packed, tab[i].b_t, tab[i].b_limbs = C.pointer(d), w.ptr, bt.ptr, p["b_limbs"]
            tab[i].bias_q, tab[i].y, tab[i].ldy = _ptr(bq), yg.ptr, ldy
            ys.append(yg)
            ins += [w, bt, bq]
        call = lambda nbytes: L.lqer_linear_forward_group(tab, len(mods), xg.ptr, dtc, M, ldx, a_cat.ptr, 1, ws.ptr, nbytes, None)
        assert call(nws - 1) == -4
        torch.cuda.synchronize()
        for yg in ys:
            yg.unchanged()
        ws.unchanged()
        assert call(nws) == 0, L.lqer_last_error()
        _check_all(ys + [ws], ins + [xg, a_cat])
        for i, (m, yg) in enumerate(zip(mods, ys)):
            ldy = m.out_features + ldy_pad
            yg.gaps_unchanged(M, m.out_features, ldy, dtype)
            _same_bits(yg.rows_view(M, m.out_features, ldy, dtype), alone[i], f"group member {i} (fill {fill:#x}) against its own forward")


# ---- split API --------------------------------------------------------------------------------------------------------------------
SPLIT_IDS = ["mx-decode2-m33", "mx-t64-m127-ldy3", "mx-t128-m300-f32", "mx-t64-m65-b64", "mx-act16-fused-m300", "w8limbs-m200",
             "int-i8-128-xch", "int-i8-128-atomic", "int-act8-fused-m1025", "int-limbs-a-m300", "w8a8-i8-128", "a16-f16-m256-dense",
             "a16-f16-m300-ldx8", "a16-limbs24-m130", "mfw-m129", "intw-m70"]


@pytest.mark.parametrize("cid", SPLIT_IDS)
def test_split_api_stays_inside_separate_buffers(lq, cid):
    """lqer_quantize_act_xa[_prep] / lqer_lowrank_xa / lqer_linear_gemm[_ld, _prepared] with xq (lqer_act_image_bytes), xaq and both
    scratches as SEPARATE guarded buffers of exactly the public sizes; the K padding of the image's live rows is zero."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    case = next(c for c in FC.CASES if c.id == cid)
    mod, xd = _module(case)
    dt, dtc = xd.dtype, ops.dtype_code(xd)
    M, K, N, es = case.M, case.K, case.N, _esz(dt)
    ldx, ldy = K + case.ldx_pad, N + case.ldy_pad
    desc = mod._desc()
    if mod._x_i8 and L.lqer_gemm_route(C.byref(desc), M, dtc) != _lib.ROUTE_I8:
        desc = mod._desc(plain=True)  # ("otherwise call them with kind LQER_Q_MXINT on the same buffers")
    base = mod(xd).clone()
    xl, al = ops.desc_limbs(desc)
    Mp, Kp, rp = L.lqer_padded_m(M), L.lqer_padded_k(K), L.lqer_padded_r(case.r)
    n_img, n_xaq = L.lqer_act_image_bytes(C.byref(desc), M), Mp * rp * 2 * al
    n_sa, n_sg = L.lqer_lowrank_xa_scratch_bytes(C.byref(desc), M), L.lqer_linear_gemm_scratch_bytes(C.byref(desc), M)
    partials = L.lqer_decode_partials(C.byref(desc), M) == 1
    dense_f16 = mod._x_f16 and ldx == K and K % 64 == 0 and (M % 256 == 0 or M <= 64)
    # (the standalone quantizer + lqer_lowrank_xa: where the forward's side product comes from the same split-K arithmetic - not where a
    # one-launch activation kernel sums x A in its own order, and not for limb weights, whose wide image is lqer_quantize_act_xa's work)
    one_launch_side = "ACT8_FUSED" in case.tune or "ACT16_FUSED" in case.tune or 1024 <= M <= 4096
    two_step = case.x_kind in ("mx", "i8") and not one_launch_side and (mod._x_i8 or ops.w_limbs(desc.w_fmt) == 1)
    variants = ["plain", "ld"] + (["prep"] if mod._x_i8 else []) + (["partials"] if partials else []) + (["two-step"] if two_step else [])
    for fill in FILLS:
        for var in variants:
            ins, a_limbs, b_limbs, _ = _forward_inputs(mod, M, desc, dtc, fill)
            x = guarded(rows_bytes(M, K, ldx, es), row_pitch_bytes=ldx * es, fill=fill, name="x").load_rows(xd, ldx)
            y = guarded(rows_bytes(M, N, ldy, es), row_pitch_bytes=ldy * es, fill=fill, name="y")
            img_pitch = n_img // Mp if n_img % Mp == 0 else 0
            xq = guarded(n_img, row_pitch_bytes=img_pitch, fill=fill, name="xq")
            xaq_ld = rp * al + (8 if var == "ld" else 0)
            xaq = guarded(Mp * xaq_ld * 2 if var == "ld" else n_xaq, row_pitch_bytes=xaq_ld * 2, fill=fill, name="xaq")
            sa = guarded(n_sa, fill=fill, name="side scratch (lqer_lowrank_xa_scratch_bytes)")
            sg = guarded(n_sg, fill=fill, name="gemm scratch (lqer_linear_gemm_scratch_bytes)")
            xq_ptr = x.ptr if dense_f16 else xq.ptr  # (the dense fp16 tensor is its own image: "the split API accepts xq == x")
            if var == "partials":  # xaq == NULL: the partial tiles stay in the side scratch, the GEMM reduces them from there
                rc = L.lqer_quantize_act_xa(C.byref(desc), x.ptr, dtc, M, ldx, _ptr(ins["a_t"]), a_limbs, xq_ptr, None, sa.ptr, n_sa, None)
                assert rc == 0, L.lqer_last_error()
                rc = L.lqer_linear_gemm(C.byref(desc), xq_ptr, M, ins["w_packed"].ptr, None, _ptr(ins["b_t"]), b_limbs, _ptr(ins["bias_q"]), y.ptr, dtc,
                                        ldy, sa.ptr, n_sa, None)
                assert rc == 0, L.lqer_last_error()
            else:
                ready = C.c_size_t(0)
                xaq_arg = xaq.ptr if case.r > 0 else None
                if var == "two-step":  # the standalone activation quantizer, then the side GEMM alone
                    f = desc.x_fmt
                    rc = (L.lqer_quantize_act_i8 if mod._x_i8 and desc.x_fmt.kind == _lib.Q_MXINT_I8 else L.lqer_quantize_act_mxint)(
                        x.ptr, dtc, M, K, ldx, C.byref(f), xq.ptr, None)
                    assert rc == 0, L.lqer_last_error()
                    if case.r > 0:
                        a2 = a_limbs if a_limbs != -2 else 1
                        rc = L.lqer_lowrank_xa(C.byref(desc), xq.ptr, M, _ptr(ins["a_t"]), a2, xaq.ptr, sa.ptr, n_sa, None)
                        assert rc == 0, L.lqer_last_error()
                elif var == "prep":
                    rc = L.lqer_quantize_act_xa_prep(C.byref(desc), x.ptr, dtc, M, ldx, _ptr(ins["a_t"]), a_limbs, xq_ptr, xaq_arg, sa.ptr, n_sa,
                                                     sg.ptr, C.byref(ready), None)
                    assert rc == 0, L.lqer_last_error()
                    assert ready.value <= n_sg
                else:
                    rc = L.lqer_quantize_act_xa(C.byref(desc), x.ptr, dtc, M, ldx, _ptr(ins["a_t"]), a_limbs, xq_ptr, xaq_arg, sa.ptr, n_sa, None)
                    assert rc == 0, L.lqer_last_error()
                _check_all([xq, xaq, sa, sg, y], [x] + list(ins.values()))
                if var == "ld":  # hand the GEMM a wider row stride: repack xaq [Mp][rp*al] -> [Mp][rp*al + 8], gaps keep the pattern
                    src = xaq.view(torch.bfloat16, Mp * rp * al).clone().view(Mp, rp * al)
                    xaq.arena.copy_(xaq.snapshot)
                    xaq.load_rows(src, xaq_ld)
                    rc = L.lqer_linear_gemm_ld(C.byref(desc), xq_ptr, M, ins["w_packed"].ptr, xaq_arg, xaq_ld, _ptr(ins["b_t"]), b_limbs,
                                               _ptr(ins["bias_q"]), y.ptr, dtc, ldy, sg.ptr, n_sg, None)
                elif var == "prep":
                    rc = L.lqer_linear_gemm_prepared(C.byref(desc), xq_ptr, M, ins["w_packed"].ptr, xaq_arg, _ptr(ins["b_t"]), b_limbs,
                                                     _ptr(ins["bias_q"]), y.ptr, dtc, ldy, sg.ptr, n_sg, ready.value, None)
                else:
                    rc = L.lqer_linear_gemm(C.byref(desc), xq_ptr, M, ins["w_packed"].ptr, xaq_arg, _ptr(ins["b_t"]), b_limbs, _ptr(ins["bias_q"]),
                                            y.ptr, dtc, ldy, sg.ptr, n_sg, None)
                assert rc == 0, L.lqer_last_error()
            _check_all([xq, sa, sg, y] + ([xaq] if var != "ld" else []), [x] + list(ins.values()) + ([xaq] if var == "ld" else []))
            y.gaps_unchanged(M, N, ldy, dt)
            _same_bits(y.rows_view(M, N, ldy, dt), base, f"{cid} [{var}, fill {fill:#x}]: y of the split calls against the module's forward")
            if not dense_f16 and case.x_kind in ("mx", "pass", "f16") and var == "plain" and Kp > K:
                # "xq [lqer_padded_m(M), lqer_padded_k(K)] (K padding zeroed ...)": columns K..Kp-1 of every limb of the rows < M
                wl = ops.w_limbs(desc.w_fmt)
                img = xq.view(torch.int16, Mp * Kp * xl * wl).view(Mp, xl * wl, Kp)
                assert not bool(img[:M, :, K:].any()), f"{cid}: the K padding of xq's live rows is not zero (fill {fill:#x})"


# ---- one-time packing -------------------------------------------------------------------------------------------------------------
def _qf(kind, w, blk, ew=8, eb=127):
    from lqer_amd._lib import QFmt

    return QFmt(kind, w, blk, ew, eb)


PACK_FMTS = {  # name: (kind, width, block, exp_width, exp_bias, block_rows)
    "mx2-b16": (1, 2, 16, 8, 127, 1), "mx3-b32": (1, 3, 32, 8, 127, 1), "mx4-b16": (1, 4, 16, 8, 127, 1), "mx4-b128": (1, 4, 128, 8, 127, 1),
    "mx4-row": (1, 4, -1, 8, 127, 1), "mx5-b16": (1, 5, 16, 8, 127, 1), "mx8-row": (1, 8, -1, 8, 127, 1), "mx8-b16": (1, 8, 16, 8, 127, 1),
    "mx4-2d-8x32": (1, 4, 32, 8, 127, 8), "mx6-2d-allx64": (1, 6, 64, 8, 127, -1),
    "int4": (4, 4, -1, 1, 7, 1), "int2": (4, 2, -1, 1, 5, 1), "mf4-e2": (5, 4, -1, 2, 7, 1), "mf4-e2-b6": (5, 4, -1, 2, 6, 1),
}


@pytest.mark.parametrize("N,K,dtype", [(1000, 200, torch.float16), (48, 1100, torch.float32), (257, 72, torch.bfloat16)])
@pytest.mark.parametrize("fname", sorted(PACK_FMTS))
def test_pack_weight_writes_its_image_and_nothing_else(lq, fname, N, K, dtype):
    """lqer_pack_weight_mxint[_2d] over N, K ragged against 256 / 64 / 16, W with a padded row stride, `scratch` of exactly
    N * ceil(K / 16) bytes: the image is written whole (the same bytes over a random fill and over 0xFF - packed bytes are read by
    kernels whose zero-padded activations do not neutralise a NaN or Inf weight), nothing else is; the unpack hook likewise."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    kind, w, blk, ew, eb, brows = PACK_FMTS[fname]
    fmt = _qf(kind, w, blk, ew, eb)
    none = _qf(0, 0, 0)
    single = _lib.LinearDesc(K, N, 0, 0, _qf(1, 8, 16), fmt, none, none, none)
    n_img = ops.linear_sizes(single, 1).w_packed
    Np, Kp = L.lqer_padded_n(N), L.lqer_padded_k(K)
    assert n_img == (Np // 16) * (Kp // 64) * 576 * (3 if kind == 1 and w > 4 else 1)
    g = torch.Generator().manual_seed(N * 7 + K)
    W = (0.02 * torch.randn(N, K, generator=g)).to(dtype).to(DEV)
    ldw, dtc, es = K + 5, ops.dtype_code(W), _esz(dtype)
    imgs, deqs = [], []
    for fill in FILLS:
        wg = guarded(rows_bytes(N, K, ldw, es), row_pitch_bytes=ldw * es, fill=fill, name="W").load_rows(W, ldw)
        out = guarded(n_img, fill=fill, name="w_packed")
        scr = guarded(N * (-(-K // 16)), fill=fill, name="pack scratch")
        if brows == 1:
            rc = L.lqer_pack_weight_mxint(wg.ptr, dtc, N, K, ldw, C.byref(fmt), out.ptr, scr.ptr, None)
        else:
            rc = L.lqer_pack_weight_mxint_2d(wg.ptr, dtc, N, K, ldw, C.byref(fmt), brows, out.ptr, scr.ptr, None)
        assert rc == 0, L.lqer_last_error()
        _check_all([out, scr], [wg])
        imgs.append(out.payload_bytes())
        deq = guarded(N * K * 4, row_pitch_bytes=K * 4, fill=fill, name="w_f32 (unpack hook)")
        img_in = guarded(n_img, fill=fill, name="w_packed (input of the unpack hook)").load(imgs[-1])
        assert L.lqer_unpack_weight_mxint(img_in.ptr, N, K, C.byref(fmt), deq.ptr, None) == 0, L.lqer_last_error()
        _check_all([deq], [img_in])
        deqs.append(deq.payload_bytes())
    _same_bits(imgs[0], imgs[1], f"{fname} {N}x{K}: packed image over a random fill against over 0xFF (unwritten bytes: none are allowed)")
    _same_bits(deqs[0], deqs[1], f"{fname} {N}x{K}: unpacked weight")
    # the Python wrapper allocates the library's size
    fmt.block_rows = brows
    assert ops.pack_weight(W, fmt).numel() == n_img
    _same_bits(ops.pack_weight(W, fmt), imgs[0], f"{fname}: ops.pack_weight against the guarded call")


@pytest.mark.parametrize("K,N,r,dtype", [(200, 1000, 20, torch.float16), (128, 48, 1, torch.float32), (1100, 257, 64, torch.bfloat16)])
def test_pack_lowrank_bias_and_the_prepared_images(lq, K, N, r, dtype):
    """lqer_pack_lowrank, lqer_pack_bias, lqer_f16_prepare, lqer_a_b16_prepare, lqer_replicate_rows: outputs at exactly their sizes,
    the same bytes over both fills."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    g = torch.Generator().manual_seed(K + N + r)
    A = (0.01 * torch.randn(K, r, generator=g)).to(dtype).to(DEV)
    B = (0.01 * torch.randn(r, N, generator=g)).to(dtype).to(DEV)
    bias = (0.01 * torch.randn(N, generator=g)).to(dtype).to(DEV)
    Wp = ops.pack_weight((0.02 * torch.randn(N, K, generator=g)).to(dtype).to(DEV), _qf(1, 4, 16))
    dtc = ops.dtype_code(A)
    mx8 = _qf(1, 8, 16)
    none = _qf(0, 0, 0)
    sz = ops.linear_sizes(_lib.LinearDesc(K, N, r, 1, mx8, _qf(1, 4, 16), mx8, mx8, mx8), 1)
    Kp, Np, rp = L.lqer_padded_k(K), L.lqer_padded_n(N), L.lqer_padded_r(r)
    keep = {}
    for fill in FILLS:
        ag, bg = _wrap_input(A, "A", fill), _wrap_input(B, "B", fill)
        a_t, b_t = guarded(sz.a_t, fill=fill, name="a_t"), guarded(sz.b_t, fill=fill, name="b_t")
        fl = guarded(8, fill=fill, align=16, name="limb_flags")
        assert L.lqer_pack_lowrank(ag.ptr, bg.ptr, dtc, K, N, r, a_t.ptr, b_t.ptr, fl.ptr, None) == 0, L.lqer_last_error()
        _check_all([a_t, b_t, fl], [ag, bg])
        limbs = fl.view(torch.int32).tolist()
        out = {"a_t": a_t.payload_bytes(), "b_t": b_t.payload_bytes(), "flags": fl.payload_bytes()}
        for name, bf in (("block_fp", _qf(1, 8, 16)), ("row", _qf(1, 8, -1)), ("pass", none), ("int", _qf(4, 8, -1, 1, 6)), ("mf", _qf(5, 8, -1, 4, 7))):
            big, bq = _wrap_input(bias, "bias", fill), guarded(sz.bias_q, fill=fill, name=f"bias_q ({name})")
            assert L.lqer_pack_bias(big.ptr, dtc, N, C.byref(bf), bq.ptr, None) == 0, L.lqer_last_error()
            _check_all([bq], [big])
            out["bias_" + name] = bq.payload_bytes()
        # lqer_f16_prepare: [rp][Kp] fp16 + the fragment-major copy; flags int32[2]
        wg, a_in = _wrap_input(Wp, "w_packed", fill), _wrap_input(a_t.view(torch.bfloat16), "a_t (input)", fill)
        a16, f2 = guarded(L.lqer_a_f16_image_bytes(K, r), fill=fill, name="a_t_f16"), guarded(8, fill=fill, align=16, name="f16 flags")
        assert L.lqer_f16_prepare(wg.ptr, N, K, a_in.ptr, limbs[0], r, a16.ptr, f2.ptr, None) == 0, L.lqer_last_error()
        _check_all([a16, f2], [wg, a_in])
        out["a16"], out["f16flags"] = a16.payload_bytes(), f2.payload_bytes()
        ab = guarded(L.lqer_a_b16_image_bytes(K, r), fill=fill, name="a_t_b16")
        assert L.lqer_a_b16_prepare(a_in.ptr, K, r, ab.ptr, None) == 0, L.lqer_last_error()
        _check_all([ab], [a_in])
        out["ab16"] = ab.payload_bytes()
        # lqer_replicate_rows: a_t rows = 3 * rp, row_bytes = Kp * 2, 3 copies
        rep = guarded(3 * sz.a_t, fill=fill, name="replicated a_t")
        assert L.lqer_replicate_rows(a_in.ptr, rep.ptr, 3 * rp, Kp * 2, 3, None) == 0, L.lqer_last_error()
        _check_all([rep], [a_in])
        out["rep"] = rep.payload_bytes()
        want = a_t.view(torch.bfloat16).view(3 * rp, 1, Kp).expand(3 * rp, 3, Kp)
        _same_bits(rep.view(torch.bfloat16), want, "lqer_replicate_rows")
        keep[fill] = out
    for k in keep[FILLS[0]]:
        _same_bits(keep[FILLS[0]][k], keep[FILLS[1]][k], f"{k} ({K}, {N}, rank {r}): over a random fill against over 0xFF")
    # the Python wrappers allocate the library's sizes
    a_t, b_t, _, _ = ops.pack_lowrank(A, B)
    assert a_t.numel() * 2 == sz.a_t and b_t.numel() * 2 == sz.b_t and ops.pack_bias(bias, mx8).numel() * 4 == sz.bias_q
    assert (Np, 3 * rp * Kp * 2) == (sz.bias_q // 4, sz.a_t)


@pytest.mark.parametrize("N,K,wname,dtype", [(1000, 200, "mx4-b128", torch.float16), (257, 128, "mx4-row", torch.bfloat16),
                                             (1000, 200, "mx8-row", torch.float16), (48, 384, "mx8-row", torch.float32)])
def test_i8_prepare_writes_its_image_and_nothing_else(lq, N, K, wname, dtype):
    """lqer_i8_prepare on a buffer of exactly lqer_linear_sizes(...).w_packed: the second image is written whole (same bytes over both
    fills), the first is not touched; both unpack hooks stay inside [N, K] fp32."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    kind, w, blk, ew, eb, _ = PACK_FMTS[wname]
    fmt = _qf(kind, w, blk, ew, eb)
    none = _qf(0, 0, 0)
    W = (0.02 * torch.randn(N, K, generator=torch.Generator().manual_seed(N + K))).to(dtype).to(DEV)
    first = ops.pack_weight(W, fmt)
    d = _lib.LinearDesc(K, N, 0, 0, _qf(3, 8, -1), fmt, none, none, none)
    n_all = ops.linear_sizes(d, 1).w_packed
    n_first = first.numel()
    off = (n_first + 255) // 256 * 256
    imgs, deqs = [], []
    for fill in FILLS:
        buf = guarded(n_all, fill=fill, name="w_packed (both images)").load(first)
        before = buf.payload_bytes()
        fl = guarded(8, fill=fill, align=16, name="i8 flags")
        assert L.lqer_i8_prepare(buf.ptr, N, K, C.byref(fmt), fl.ptr, None) == 0, L.lqer_last_error()
        _check_all([buf, fl], [])
        assert fl.view(torch.int32).tolist()[0] == 0
        now = buf.payload_bytes()
        _same_bits(now[:n_first], before[:n_first], "the sign-magnitude image in front of the int8 image")
        _same_bits(now[n_first:off], before[n_first:off], "the alignment gap between the two images")
        imgs.append(now[off:])
        src = guarded(n_all, fill=fill, name="w_packed (input of the unpack hook)").load(now)
        deq = guarded(N * K * 4, row_pitch_bytes=K * 4, fill=fill, name="w_f32 (int8 unpack hook)")
        assert L.lqer_unpack_weight_i8_fmt(src.ptr, N, K, C.byref(fmt), deq.ptr, None) == 0, L.lqer_last_error()
        if w <= 4:
            deq2 = guarded(N * K * 4, row_pitch_bytes=K * 4, fill=fill, name="w_f32 (lqer_unpack_weight_i8)")
            assert L.lqer_unpack_weight_i8(src.ptr, N, K, deq2.ptr, None) == 0, L.lqer_last_error()
            _check_all([deq2], [src])
            _same_bits(deq2.payload_bytes(), deq.payload_bytes(), "the two int8 unpack hooks")
        _check_all([deq], [src])
        deqs.append(deq.payload_bytes())
        _same_bits(deq.view(torch.float32), ops.unpack_weight(first, N, K, fmt), "the int8 image's weights against the sign-magnitude image's")
    _same_bits(imgs[0], imgs[1], f"{wname} {N}x{K}: int8 weight image over a random fill against over 0xFF (unwritten bytes: none are allowed)")
    _same_bits(deqs[0], deqs[1], "unpacked int8 image")
    ok, pybuf = ops.i8_prepare(first, N, K, fmt)
    assert ok and pybuf.numel() == n_all


# ---- standalone quantizers --------------------------------------------------------------------------------------------------------
QUANT_FMTS = {"mx8-b16": (1, 8, 16, 8, 127), "mx4-b32": (1, 4, 32, 8, 127), "mx8-row": (1, 8, -1, 8, 127), "mx6-e4": (1, 6, 16, 4, 7),
              "int8": (4, 8, -1, 1, 4), "uint6": (4, 6, -1, 0, 3), "mf8-e4": (5, 8, -1, 4, 7), "mf4-e2": (5, 4, -1, 2, 1)}


@pytest.mark.parametrize("rows,cols,pad,dtype", [(5, 200, 5, torch.float16), (300, 72, 8, torch.float32), (1, 1100, 0, torch.bfloat16), (67, 16, 3, torch.float16)])
@pytest.mark.parametrize("fname", sorted(QUANT_FMTS))
def test_quantize_mxint_outputs_alone_and_together(lq, fname, rows, cols, pad, dtype):
    """lqer_quantize_mxint: deq [rows, cols] fp32, codes [rows, cols] int8, exps [rows, ceil(cols / L)] int8 - each alone and all together,
    ld > cols, cols not a multiple of the block, all three kinds: every output whole, nothing else written, the same bits either way."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    fmt = _qf(*QUANT_FMTS[fname])
    x = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)) * 3).to(dtype).to(DEV)
    ld, es, dtc = cols + pad, _esz(dtype), ops.dtype_code(x)
    blk = cols if fmt.block <= 0 or fmt.block >= cols else fmt.block
    nblk = -(-cols // blk)
    has_exps = fmt.kind == _lib.Q_MXINT
    base = ops.quantize_mxint(x, fmt, want=("deq", "codes") + (("exps",) if has_exps else ()))
    sizes = {"deq": rows * cols * 4, "codes": rows * cols, "exps": rows * nblk}
    combos = [("deq",), ("codes",), ("deq", "codes")] + ([("exps",), ("deq", "codes", "exps")] if has_exps else [])
    for fill in FILLS:
        for want in combos:
            xg = guarded(rows_bytes(rows, cols, ld, es), row_pitch_bytes=ld * es, fill=fill, name="x").load_rows(x, ld)
            outs = {k: guarded(sizes[k], fill=fill, row_pitch_bytes={"deq": cols * 4, "codes": cols, "exps": nblk}[k], name=k) for k in want}
            rc = L.lqer_quantize_mxint(xg.ptr, dtc, rows, cols, ld, C.byref(fmt), _ptr(outs.get("deq")), _ptr(outs.get("codes")), _ptr(outs.get("exps")), None)
            assert rc == 0, L.lqer_last_error()
            _check_all(list(outs.values()), [xg])
            for k, gd in outs.items():
                _same_bits(gd.payload_bytes(), base[k], f"{fname} {rows}x{cols} ld {ld}: {k} of {want} (fill {fill:#x}) against ops.quantize_mxint")


@pytest.mark.parametrize("batches,rows,cols,R,Lc,dtype", [(2, 37, 200, 8, 16, torch.float16), (1, 300, 72, -1, 32, torch.float32), (3, 5, 48, 4, -1, torch.bfloat16)])
def test_quantize_tiles_act_and_i8_images(lq, batches, rows, cols, R, Lc, dtype):
    """lqer_quantize_mxint_tiles (amax_scratch of exactly one float per tile), lqer_quantize_act_mxint (image [Mp][Kp] bf16) and
    lqer_quantize_act_i8 (image [Mp][K padded to 128] int8, 256-byte aligned, then Mp fp32 row scales)."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    fmt = _qf(1, 8, 16)
    x = (torch.randn(batches, rows, cols, generator=torch.Generator().manual_seed(rows)) * 2).to(dtype).to(DEV)
    dtc, es = ops.dtype_code(x), _esz(dtype)
    Re, Le = (rows if R <= 0 or R > rows else R), (cols if Lc <= 0 or Lc > cols else Lc)
    ntiles = batches * (-(-rows // Re)) * (-(-cols // Le))
    fmt_t = ops.make_qfmt(dict(name="block_fp", width=8, block_size=[R, Lc], skip_first_dim=True), "x")
    base = ops.quantize_act_tiles(x, fmt_t).float()
    x2 = x[0]
    M, K = x2.shape
    Mp, Kp, K8 = L.lqer_padded_m(M), L.lqer_padded_k(K), -(-K // 128) * 128
    img_b = ops.quantize_act(x2, fmt)
    per_row = _qf(1, 8, -1)
    i8_b, sc_b = ops.quantize_act_i8(x2, per_row)
    n_i8 = (Mp * K8 + 255) // 256 * 256
    assert i8_b.numel() == Mp * K8 and sc_b.numel() == Mp  # (the wrapper's own layout formula: the header's)
    for fill in FILLS:
        xg = _wrap_input(x, "x", fill)
        deq, am = guarded(batches * rows * cols * 4, row_pitch_bytes=cols * 4, fill=fill, name="deq (tiles)"), guarded(ntiles * 4, fill=fill, name="amax_scratch")
        assert L.lqer_quantize_mxint_tiles(xg.ptr, dtc, batches, rows, cols, C.byref(fmt_t), Re, Le, deq.ptr, am.ptr, None) == 0, L.lqer_last_error()
        _check_all([deq, am], [xg])
        _same_bits(deq.view(torch.float32), base, f"lqer_quantize_mxint_tiles (fill {fill:#x})")
        ldx = K + 5
        x2g = guarded(rows_bytes(M, K, ldx, es), row_pitch_bytes=ldx * es, fill=fill, name="x").load_rows(x2, ldx)
        img = guarded(Mp * Kp * 2, row_pitch_bytes=Kp * 2, fill=fill, name="xq (lqer_quantize_act_mxint)")
        assert L.lqer_quantize_act_mxint(x2g.ptr, dtc, M, K, ldx, C.byref(fmt), img.ptr, None) == 0, L.lqer_last_error()
        _check_all([img], [x2g])
        _same_bits(img.view(torch.bfloat16).view(Mp, Kp)[:M], img_b[:M], f"lqer_quantize_act_mxint rows < M (fill {fill:#x})")
        i8 = guarded(n_i8 + Mp * 4, row_pitch_bytes=K8, fill=fill, name="xq_i8 (image + row scales)")
        assert L.lqer_quantize_act_i8(x2g.ptr, dtc, M, K, ldx, C.byref(per_row), i8.ptr, None) == 0, L.lqer_last_error()
        _check_all([i8], [x2g])
        _same_bits(i8.view(torch.int8, Mp * K8).view(Mp, K8)[:M], i8_b[:M], f"lqer_quantize_act_i8 mantissas of rows < M (fill {fill:#x})")
        _same_bits(i8.view(torch.float32, Mp, n_i8)[:M], sc_b[:M], f"lqer_quantize_act_i8 row scales of rows < M (fill {fill:#x})")


# ---- attention products and calibration statistics ----------------------------------------------------------------------------------
@pytest.mark.parametrize("b,S1,K,S2,xblk,yblk,dtype,ytrans", [(2, 37, 72, 50, 16, 16, torch.float16, True), (3, 130, 128, 200, 16, 16, torch.bfloat16, False),
                                                               (2, 37, 80, 48, -1, 16, torch.float16, False), (1, 65, 64, 129, 32, -1, torch.float32, False)])
def test_matmul_q_stays_inside_out_and_workspace(lq, b, S1, K, S2, xblk, yblk, dtype, ytrans):
    """lqer_matmul_q: `out` dense at its exact size, workspace from lqer_matmul_q_workspace_bytes_fmt exactly, strided x (x_rs > K), the
    transposed view of y, blocks of 16 and others."""
    from lqer_amd import _lib, functional, ops

    L = _lib.lib()
    fx, fy = _qf(1, 8, xblk), _qf(1, 8, yblk)
    g = torch.Generator().manual_seed(S1 + S2)
    x = torch.randn(b, S1, K, generator=g).to(dtype).to(DEV)
    y = torch.randn(b, K, S2, generator=g).to(dtype).to(DEV)
    base = functional._matmul_fused(x, y, fx, fy)
    es, dtc = _esz(dtype), ops.dtype_code(x)
    x_rs = K + 8
    nws = L.lqer_matmul_q_workspace_bytes_fmt(b, S1, K, S2, C.byref(fx), C.byref(fy))
    for fill in FILLS:
        xg = guarded(rows_bytes(b * S1, K, x_rs, es), row_pitch_bytes=x_rs * es, fill=fill, name="x").load_rows(x.reshape(b * S1, K), x_rs)
        if ytrans:  # y[b][k][j] at b S2 K + j K + k: the transposed VIEW of a [b, S2, K] tensor (Q K^T)
            yg = _wrap_input(y.transpose(1, 2).contiguous(), "y (stored [b, S2, K])", fill)
            ystr = (S2 * K, 1, K)
        else:
            yg, ystr = _wrap_input(y, "y", fill), (K * S2, S2, 1)
        out = guarded(b * S1 * S2 * es, row_pitch_bytes=S2 * es, fill=fill, name="out")
        ws = guarded(nws, fill=fill, name="matmul_q workspace")
        call = lambda nb: L.lqer_matmul_q(xg.ptr, yg.ptr, out.ptr, dtc, b, S1, K, S2, S1 * x_rs, x_rs, ystr[0], ystr[1], ystr[2], C.byref(fx), C.byref(fy),
                                          ws.ptr, nb, None)
        assert call(nws - 1) == -4
        assert call(nws) == 0, L.lqer_last_error()
        _check_all([out, ws], [xg, yg])
        _same_bits(out.view(dtype), base, f"lqer_matmul_q (fill {fill:#x}) against lqer_amd.functional")


@pytest.mark.parametrize("M,K,pad,off,dtype", [(37, 200, 0, 0, torch.float16), (300, 72, 5, 0, torch.float32), (1, 1100, 0, 2, torch.bfloat16),
                                               (1025, 48, 3, 6, torch.float16)])
def test_col_abs_stats_stays_inside_its_outputs(lq, M, K, pad, off, dtype):
    """lqer_col_abs_stats: run / absmax of [K] fp32, count of [1] int32, workspace exact; ldx > K and an x that is not 16-byte aligned."""
    from lqer_amd import _lib, ops

    L = _lib.lib()
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dtype).to(DEV)
    run0 = torch.rand(K, generator=torch.Generator().manual_seed(K)).to(DEV)
    b = ops.col_abs_stats(x, run=run0.clone(), want_absmax=True, threshold=2.5)
    es, dtc, ldx = _esz(dtype), ops.dtype_code(x), K + pad
    nws = L.lqer_col_abs_stats_workspace_bytes(M, K)
    for fill in FILLS:
        # x at `off` bytes into a guarded payload: an element-aligned, not 16-byte aligned tensor
        xg = guarded(off + rows_bytes(M, K, ldx, es), row_pitch_bytes=ldx * es, fill=fill, name="x")
        xg.payload[off:].view(dtype).as_strided((M, K), (ldx, 1)).copy_(x)
        xg.snapshot = xg.arena.clone()
        run = guarded(K * 4, fill=fill, name="run_absmean_max").load(run0)
        run.snapshot = run.arena.clone()
        am, cnt = guarded(K * 4, fill=fill, name="col_absmax"), guarded(4, fill=fill, align=16, name="n_cols_ge")
        ws = guarded(nws, fill=fill, align=16, name="col_abs_stats workspace")
        call = lambda nb: L.lqer_col_abs_stats(xg.ptr + off, dtc, M, K, ldx, run.ptr, am.ptr, 2.5, cnt.ptr, ws.ptr, nb, None)
        assert call(nws - 1) == -4 if nws else True
        assert call(nws) == 0, L.lqer_last_error()
        _check_all([run, am, cnt, ws], [xg])
        _same_bits(run.view(torch.float32), b.run, f"run (fill {fill:#x})")
        _same_bits(am.view(torch.float32), b.absmax, f"absmax (fill {fill:#x})")
        _same_bits(cnt.view(torch.int32), b.count, f"count (fill {fill:#x})")

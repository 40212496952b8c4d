"""Host-side size contracts of the C ABI (include/lqer_hip.h), no GPU: what lqer_linear_sizes and the public scratch-size functions
report over a grid of descriptors - monotone in the token count, enough for the carving a split-API caller makes from the public
functions, equal to the layout formulae the header states - and the route coverage of the guard-zone case table
(tests/_footprint_cases.py) that tests/test_gpu_footprint.py runs on the GPU."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _footprint_cases as FC  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _fmt_sets():
    """(name, x, w, a_out, b_out) format sets of the grid."""
    from lqer_amd import _lib
    from lqer_amd._lib import QFmt

    mx = lambda w, blk: QFmt(_lib.Q_MXINT, w, blk, 8, 127)
    pt = lambda w: QFmt(_lib.Q_PASSTHROUGH, w, 0, 8, 127)
    i8 = QFmt(_lib.Q_MXINT_I8, 8, -1, 8, 127)
    return [
        ("mxint16", mx(8, 16), mx(4, 16), mx(8, 16), mx(8, 16)),                      # MXINT blocks of 16
        ("mxint16-bout64", mx(8, 16), mx(4, 16), mx(8, 16), mx(8, 64)),               # B_out blocks of 64
        ("mxint16-boutrow", mx(8, 16), mx(4, 16), mx(8, 16), mx(8, -1)),              # B_out per row
        ("int-i8-w4", i8, mx(4, 128), mx(8, -1), mx(8, -1)),                          # the INT template on the int8 route, 4-bit weights
        ("int-i8-w8", i8, mx(8, -1), mx(8, -1), mx(8, -1)),                           # ... 8-bit weights (the image of codes)
        ("pass11", pt(11), mx(4, 128), pt(16), pt(0)),                                # pass-through, fp16 as two limbs
        ("pass24", pt(24), mx(4, 128), pt(24), pt(0)),                                # pass-through, fp32 as three limbs
        ("pass-f16", QFmt(_lib.Q_PASSTHROUGH_F16, 11, 0, 8, 127), mx(4, 128), pt(16), pt(0)),
        ("w8-limbs", mx(8, 16), mx(8, 16), mx(8, 16), mx(8, 16)),                     # 8-bit limb weights
        ("minifloat", QFmt(_lib.Q_MINIFLOAT, 8, -1, 4, 7), QFmt(_lib.Q_MINIFLOAT, 4, -1, 2, 7), QFmt(_lib.Q_MINIFLOAT, 8, -1, 4, 7),
         QFmt(_lib.Q_MINIFLOAT, 8, -1, 4, 7)),
    ]


KS = (128, 200, 1024, 1100, 4096)   # ragged against 64 and 128: 200, 1100
NS = (48, 1000, 4096, 11008)        # ragged against 256 and 32: 48, 1000
RANKS = (0, 1, 16, 20, 32, 64, 100, 128)
TOKENS = sorted({max(0, c + d) for c in (0, 8, 64, 128, 256, 512, 1024, 2048, 4096) for d in (-2, -1, 0, 1, 2)} | {3000, 4352})

align256 = lambda v: (v + 255) // 256 * 256


def _grid():
    from lqer_amd import _lib

    none = _lib.QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
    for name, fx, fw, fa, fb in _fmt_sets():
        for K in KS:
            for N in NS:
                for r in RANKS:
                    yield name, _lib.LinearDesc(K, N, r, 1, fx, fw, none, fa, fb)


def _sizes(lib, d, m):
    from lqer_amd import _lib

    sz = _lib.LinearSizes()
    rc = lib.lqer_linear_sizes(C.byref(d), m, C.byref(sz))
    assert rc == 0, (rc, lib.lqer_last_error())
    return sz


def test_workspace_is_monotone_and_covers_the_split_carving(lib):
    """The forward compares the caller's bytes with the size for M, so the header's promise "workspace >=
    lqer_linear_sizes(...).workspace for m_max >= M" rests on the size never decreasing in the token count; and a caller of the split
    API carves image | xaq | scratch from the public functions: the workspace must hold that too."""
    n = 0
    for name, d in _grid():
        al = C.c_int(1)
        xl = C.c_int(1)
        assert lib.lqer_desc_limbs(C.byref(d), C.byref(xl), C.byref(al)) == 0
        rp = lib.lqer_padded_r(d.rank)
        prev = 0
        for m in TOKENS:
            ws = _sizes(lib, d, m).workspace
            assert ws >= prev, f"{name} K={d.in_features} N={d.out_features} r={d.rank}: workspace({m}) = {ws} < workspace of fewer tokens {prev}"
            prev = ws
            Mp = lib.lqer_padded_m(m)
            carve = (lib.lqer_act_image_bytes(C.byref(d), m) + align256(Mp * rp * 2 * al.value)
                     + max(lib.lqer_lowrank_xa_scratch_bytes(C.byref(d), m), lib.lqer_linear_gemm_scratch_bytes(C.byref(d), m)))
            assert ws >= carve, f"{name} K={d.in_features} N={d.out_features} r={d.rank} M={m}: workspace {ws} < split carving {carve}"
            n += 1
    assert n > 50000


def test_scratch_sizes_are_monotone(lib):
    """The split calls take scratch sized for m_max >= M as well."""
    for name, d in _grid():
        pa = pg = pi = 0
        for m in TOKENS:
            a, g, i = (lib.lqer_lowrank_xa_scratch_bytes(C.byref(d), m), lib.lqer_linear_gemm_scratch_bytes(C.byref(d), m),
                       lib.lqer_act_image_bytes(C.byref(d), m))
            assert a >= pa and g >= pg and i >= pi, (name, d.in_features, d.out_features, d.rank, m)
            pa, pg, pi = a, g, i


def test_side_scratch_holds_the_fused_kernels_partial_tiles(lib):
    """The one-launch quantizer + split-K kernel (csrc/quant_xa16.hip, xa_fused_plan) leaves one fp32 partial tile of 32 token rows x
    padded rank per 256 k and row group in the side scratch, and checks the caller's bytes on the host: a size function that reports
    one row group less sends every forward of such a shape to the slower separate steps without an error - invisible to a guard zone
    (nothing overruns) and to the values (same bits).  From about K = 4096 and a few thousand tokens this plan, not the split-K bound,
    decides the size: held here to the last tile."""
    from lqer_amd import _lib

    mx = lambda w, blk: _lib.QFmt(_lib.Q_MXINT, w, blk, 8, 127)
    none = _lib.QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
    tight = 0
    for K in KS + (11008,):
        Kp = lib.lqer_padded_k(K)
        for r in (16, 20, 32, 64, 128):
            d = _lib.LinearDesc(K, 256, r, 0, mx(8, 16), mx(4, 16), none, mx(8, 16), mx(8, 16))
            rp = lib.lqer_padded_r(r)
            for m in TOKENS + [8192, 16384]:
                need = -(-m // 32) * -(-Kp // 256) * 32 * rp * 4
                got = lib.lqer_lowrank_xa_scratch_bytes(C.byref(d), m)
                assert got >= need, f"side scratch (lqer_lowrank_xa_scratch_bytes) K={K} rank={r} M={m}: {got} B < {need} B of partial tiles"
                tight += got == need
    assert tight > 0  # (the grid reaches shapes where the bound is exact)


def test_group_workspace_covers_the_one_launch_decode_routes_scratch(lib):
    """The one-launch decode kernel runs, for a single Linear, inside lqer_linear_forward on the side-path scratch of M tokens
    (lqer_lowrank_xa_scratch_bytes) and, for a group, on lqer_group_workspace_bytes: the group size of the same K and padded rank
    must fit the single forward's scratch (or the forward would fall through to the two-launch route for lack of room) and the
    single forward's workspace."""
    from lqer_amd import _lib

    mx = lambda w, blk: _lib.QFmt(_lib.Q_MXINT, w, blk, 8, 127)
    none = _lib.QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
    for K in KS + (11008,):
        for r in (1, 16, 20, 32, 48, 64):
            d = _lib.LinearDesc(K, 256, r, 0, mx(8, 16), mx(4, 16), none, mx(8, 16), mx(8, 16))
            rp = lib.lqer_padded_r(r)
            for m in range(1, 9):
                assert lib.lqer_decode_partials(C.byref(d), m) == 1
                g = lib.lqer_group_workspace_bytes(K, rp)
                assert g > 0 and g % 256 == 0
                assert g <= align256(lib.lqer_lowrank_xa_scratch_bytes(C.byref(d), m)), (K, r, m)
                assert g <= _sizes(lib, d, m).workspace
            # a group of members: the sum of the padded ranks
            assert lib.lqer_group_workspace_bytes(K, 2 * rp) >= lib.lqer_group_workspace_bytes(K, rp)


def test_operand_sizes_equal_the_headers_layout_formulae(lib):
    from lqer_amd import _lib

    for name, d in _grid():
        K, N, r = d.in_features, d.out_features, d.rank
        Kp, Np, rp = lib.lqer_padded_k(K), lib.lqer_padded_n(N), lib.lqer_padded_r(r)
        xl, al = C.c_int(1), C.c_int(1)
        lib.lqer_desc_limbs(C.byref(d), C.byref(xl), C.byref(al))
        xl, al = xl.value, al.value
        sz = _sizes(lib, d, 1)
        # "Panel (n/16, k/64) = 16 rows x 32 B codes followed by 16 x 4 exponent bytes" / LQER_PANEL_BYTES 576;
        # "w_packed is [Np / 16][3][Kp / 64] panels (lqer_linear_sizes: three times the 4-bit size)" for widths 5..8;
        # "w_packed / a_t must hold L copies of the packed image along k" for pass-through activations
        wl = 3 if (d.w_fmt.kind == _lib.Q_MXINT and d.w_fmt.width > 4) else 1
        panels = (Np // 16) * (Kp // 64) * 576 * wl
        if d.x_fmt.kind == _lib.Q_MXINT_I8:
            # "w_packed = the 4-bit sign-magnitude image of lqer_pack_weight_mxint followed (256-byte aligned) by a second image"
            assert sz.w_packed > align256(panels), (name, K, N)
            K8 = (K + 127) // 128 * 128
            if wl == 3:  # "per (256-row tile, 64-k half-step) 256 rows x 64 B, then one scale per row"
                assert sz.w_packed == align256(panels) + (Np // 256) * (K8 // 64) * 256 * 64 + Np * 4, (name, K, N)
        else:
            assert sz.w_packed == panels * xl, (name, K, N)
        # "a_t [3][rp][Kp]" bf16, L copies along k;  "b_t [3][Np][rp]", LA copies along r;  "bias_q ... fp32 [Np]"
        assert sz.a_t == 3 * rp * Kp * 2 * xl, (name, K, N, r)
        assert sz.b_t == 3 * Np * rp * 2 * al, (name, K, N, r)
        assert sz.bias_q == Np * 4
        # "xq is [Mp][L*Kp]" bf16; 5..8-bit weights: "[padded M][padded K x activation limbs x weight limbs] bf16, plus ... the
        # single-copy image behind it"
        for m in (1, 300, 2048):
            Mp = lib.lqer_padded_m(m)
            one = align256(Mp * Kp * 2 * xl)
            img = lib.lqer_act_image_bytes(C.byref(d), m)
            assert img == (one if wl == 1 else align256(one * wl) + one), (name, K, N, m)
            if d.x_fmt.kind == _lib.Q_MXINT_I8:
                # "[Mp][K padded to 128] mantissas followed (256-byte aligned) by Mp fp32 row scales; never larger than the bf16 image"
                assert align256(Mp * ((K + 127) // 128 * 128)) + Mp * 4 <= img
    # the images of lqer_f16_prepare / lqer_a_b16_prepare: "[rp][Kp] fp16 ... followed by its FRAGMENT-MAJOR copy ... over
    # ceil(K / 128) * 128 columns";  "limb 0 ... ([rp][Kp] bf16) ... and ... its fragment-major copy behind it"
    for K in KS:
        for r in RANKS[1:]:
            Kp, rp, K8 = lib.lqer_padded_k(K), lib.lqer_padded_r(r), (K + 127) // 128 * 128
            assert lib.lqer_a_f16_image_bytes(K, r) == rp * (Kp + K8) * 2
            assert lib.lqer_a_b16_image_bytes(K, r) == 2 * rp * Kp * 2


def test_the_case_table_reaches_every_route_for_two_dtypes(lib):
    """tests/test_gpu_footprint.py runs this table: every GEMM route and tile height must be in it for at least two element types,
    and every row's expectation must be what the library's host logic says."""
    from lqer_amd import _lib, ops

    names = {_lib.ROUTE_SMALLM: FC.S, _lib.ROUTE_TILE128: FC.T128, _lib.ROUTE_TILE256: FC.T256, _lib.ROUTE_I8: FC.I8}
    code = {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}
    seen = {}
    ids = [c.id for c in FC.CASES]
    assert len(set(ids)) == len(ids)
    for c in FC.CASES:
        d = FC.host_desc(c)
        route = lib.lqer_gemm_route(C.byref(d), c.M, code[c.dtype])
        assert route >= 0, (c.id, lib.lqer_last_error())
        rows = lib.lqer_gemm_tile_rows(C.byref(d), c.M, code[c.dtype])
        if c.x_kind == "i8" and route != _lib.ROUTE_I8:
            # (the forward switches such a call to the bf16 kernels on the same buffers: ask for that descriptor's tile)
            d.x_fmt.kind = _lib.Q_MXINT
            rows = lib.lqer_gemm_tile_rows(C.byref(d), c.M, code[c.dtype])
        assert (names[route], rows) == (c.route, c.rows), f"{c.id}: the library says {names[route]} / {rows} rows"
        seen.setdefault((c.route, c.rows), set()).add(c.dtype)
        assert ops.linear_sizes(d, c.M).workspace > 0
    for pair in FC.REQUIRED_ROUTES:
        assert len(seen.get(pair, ())) >= 2, f"route {pair}: dtypes {sorted(seen.get(pair, ()))}"
    # the one-launch decode kernel (up to 8 tokens, 16-byte rows) and the two-launch decode route are both in the table
    dec = [c for c in FC.CASES if c.cfg.startswith("mx") and c.route == FC.S and c.r > 0]
    assert any(c.M <= 8 and c.ldx_pad % 8 == 0 for c in dec) and any(c.M > 8 or c.ldx_pad % 8 for c in dec)

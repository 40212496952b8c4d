"""The 256-row tile kernel of the fused GEMM (csrc/gemm_w4a8_m256.hip, k_lqer_gemm_m256), bit for bit, over every output element.

It compiles gemm_tile.h with the 128-row kernels (swizzle, tile order, weight-piece offsets, descriptor words, the LOAD statements), so
every change to them changes this kernel; the plan sends it every large-M shape.  Two references, both computed here:

 1. the exact product (no side path): x and W quantized by the oracle, xq Wq^T in float64, rounded ONCE to the output type, equal over
    all M x N elements - valid while every fp32 partial sum is exact in any order, which each case asserts before it compares
    (tests/_gemm256_cases.py: sum |xq| |Wq| < 2^24 u).  K = 64 .. 320 give 1 .. 5 k-steps (vmcnt(0) / vmcnt(5) in front of the loop,
    every exit of the loop unrolled by the ring size 3), K = 200 a zero-padded k-step, K = 1024 sixteen steps of steady state; N = 2304,
    2280 (last wave narrow) and 2276 (every 16-bit store narrow, guarded float4); M = 4098 (a ragged 17th row tile; 153 tiles).
 2. every instantiation against the 128-row kernel (pinned by tests/test_gpu_gemm128_golden.py): the same module on the same x in
    slices of 256 rows, each asserted to run on 128-row tiles, equal over ALL rows - rows are independent in every quantizer used.

Every case asserts the route (LQER_ROUTE_TILE256, 256 rows) before it runs, and prints one line: route, tile rows, the exactness margin
or the number of slices, the count of differing elements.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import copy
import math

import pytest
import torch

import _gemm256_cases as G

pytestmark = pytest.mark.gpu

from oracle import lqer_oracle as O  # the checker

DEV = G.DEV


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import lqer_amd

    return lqer_amd


def _assert_tile256(mod, M, dtype):
    from lqer_amd import _lib

    route, rows = G.route_of(mod, M, dtype)
    assert route == _lib.ROUTE_TILE256 and rows == 256, (route, rows)
    return route, rows


# ---- 1. the exact product ---------------------------------------------------------------------------------------------------------------
EXACT_CASES = ([(g, K, "f32", False) for g in ("A", "A2280", "A2276") for K in G.EXACT_KS] +
               [(g, K, dt, False) for g in ("A", "A2280", "A2276") for K in (64, 200, 1024) for dt in ("f16", "bf16")] +
               [("A2280", 1024, "f32", True), ("A2276", 200, "bf16", True), ("A", 320, "f16", True)])  # bias = one more exact term


@pytest.mark.parametrize("geom,K,dt,bias", EXACT_CASES)
def test_exact_product_every_element(lq, geom, K, dt, bias):
    from bench import MXINT_Q

    M, N = G.GEOM[geom]
    dtype = G.DTYPES[dt]
    op = G.exact_operands(K)
    # the condition of the comparison, asserted (never a reason to skip): every partial sum in any order is exact in fp32
    margin = op["margin"]
    if bias:
        bq, on_grid, margin = G.exact_bias(K, N)
        assert on_grid
    assert margin < 1.0, (K, margin)
    mod = lq.LinearFlexible(K, N, bias=bias, q_config=dict(MXINT_Q, name="flexible"))
    sd = {"weight": op["W"][:N]}
    if bias:
        sd["bias"] = op["b"][:N]
    mod.load_state_dict(sd)
    mod = mod.to(DEV).to(dtype)
    route, rows = _assert_tile256(mod, M, dtype)
    y = mod(op["x"].to(dtype).to(DEV))
    want = op["ref32"][:, :N]  # (fp32 holds the exact sum)
    if bias:
        want = (want.double() + bq.to(DEV).double()[None, :]).float()  # round(bias + sum): still below 2^24 u, exact
    want = want.to(dtype)  # the one rounding
    ndiff = int((y != want).sum())
    print(f"gemm256 exact {geom} {M}x{N} K{K} {dt}{' bias' if bias else ''}: route {route} rows {rows} u 2^{int(math.log2(op['u']))} "
          f"margin {margin:.4f} differing {ndiff}")
    assert y.shape == want.shape and torch.equal(y, want)
    if bias:  # like the reference, the parameter now holds b_quantizer(bias): the term that was added
        assert torch.equal(mod.bias.detach().float().cpu(), bq)


# ---- 2. every instantiation against the 128-row kernel, all rows ------------------------------------------------------------------------
def _full_and_slices(mod, xd, M, dtype):
    """y of the full forward (256-row tiles, asserted) and the concatenation of the forwards over 256-row slices (128-row tiles, asserted)."""
    from lqer_amd import _lib

    route, rows = _assert_tile256(mod, M, dtype)
    y = mod(xd).clone()
    ys = torch.empty_like(y)
    starts = G.slice_starts(M)
    try:
        mod.tuning = _lib.TUNE_TILE_ROWS_128  # (64-row tiles would be chosen at 256 rows; tests/test_gpu_tile_rows.py holds them to these)
        for s in starts:
            assert G.route_of(mod, 256, dtype) == (_lib.ROUTE_TILE128, 128)
            ys[s:s + 256] = mod(xd[s:s + 256])
    finally:
        mod.tuning = 0
    return y, ys, route, rows, len(starts)


@pytest.mark.parametrize("cid", [c[0] for c in G.SIDE_CASES])
def test_256_row_tiles_equal_128_row_tiles_on_all_rows(lq, cid):
    mod, xd, c = G.side_case(cid)
    M, dtype = c["M"], c["dtype"]
    y, ys, route, rows, nsl = _full_and_slices(mod, xd, M, dtype)
    bad_rows = (y != ys).any(dim=1)
    ndiff = int((y != ys).sum())
    excused = 0
    if cid.startswith("8-int-limbs") and ndiff:
        # unquantized A: the order of the sums of x A may depend on M; rows of the exact x A within D ulps of an A_out tie (or of a power
        # of two at the block maximum) may come out one step apart - those alone are excused, at most 2 % of M
        from _envelope import tie_rows

        h = lambda t: t.to(dtype).float()
        qx = O.get_quantizer(c["qc"]["x_quantizer"])
        s64 = qx(h(c["x"])).double().numpy() @ h(c["A"]).double().numpy()
        ties = torch.from_numpy(tie_rows(s64, c["r"], 7, max(16.0, math.sqrt(c["K"])))).to(DEV)
        excused = int(ties.sum())
        assert excused <= 0.02 * M, excused
        bad_rows &= ~ties
    print(f"gemm256 vs 128-row tiles {cid} {M}x{c['N']} K{c['K']} r{c['r']} {dtype}: route {route} rows {rows} slices {nsl} "
          f"differing {ndiff} in {int((y != ys).any(dim=1).sum())} rows, excused rows {excused}")
    assert not bool(bad_rows.any()), (ndiff, bad_rows.nonzero().flatten()[:8].tolist())
    if cid == "12-steady-state":
        # the chain 256 -> 128 -> oracle at one long K: a seeded sample of 512 rows at the bars of tests/test_gpu_tile_rows.py
        idx = torch.randperm(M, generator=torch.Generator().manual_seed(12))[:512].sort().values
        h = lambda t: None if t is None else t.to(dtype).float()
        ref = O.lqer_linear_forward(h(c["x"][idx]), h(c["W"]), h(c["b"]), h(c["A"]), h(c["B"]), c["qc"])
        err = float((y[idx.to(DEV)].float().cpu() - ref).norm() / ref.norm())
        print(f"gemm256 {cid}: rel-L2 vs oracle on 512 rows {err:.3e}")
        assert err <= (4e-3 if dtype == torch.bfloat16 else 1e-3), err


# ---- 4. graph replay and two streams (barrier-phased wave groups, 125952 B of LDS: one workgroup per CU) ---------------------------------
def test_256_row_tiles_under_graph_replay(lq):
    mod, xd, c = G.side_case("3-r64-narrow-f32")
    _assert_tile256(mod, c["M"], c["dtype"])
    y0 = mod(xd).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mod(xd)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y1 = mod(xd)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y1, y0)


def test_256_row_tiles_on_two_streams(lq):
    """Forwards issued alternately on two streams (each module copy with its own workspace) give the bits of the forwards alone."""
    mod, xd, c = G.side_case("3-r64-narrow-f32")
    xs = [xd, (xd * 0.5).contiguous()]
    mods = [mod, copy.deepcopy(mod)]
    for m in mods:
        _assert_tile256(m, c["M"], c["dtype"])
    ref = [mods[i](xs[i]).clone() for i in (0, 1)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    outs = [[], []]
    for _ in range(12):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                outs[i].append(mods[i](xs[i]))
    torch.cuda.synchronize()
    for i in (0, 1):
        for y in outs[i]:
            assert torch.equal(y, ref[i])

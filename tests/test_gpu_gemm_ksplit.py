"""The k split of the 128-row tile kernel (csrc/gemm_w4a8.hip, KSPLIT): the two waves of a SIMD share 128 x 64 outputs, each
takes two of a k-step's four 16-deep slices, the deferred side product is held 64 rows at a time, and the pairs exchange partial sums
through LDS behind the main loop.  Against the kernel it replaces (LQER_TUNE_NO_KSPLIT, k_lqer_gemm_nks: every wave takes all four slices of its own
32 columns) bit for bit - on MXINT operands every partial sum is exact in fp32, so two chains and an add give the same bits - and
against the oracle (reference quantized_layers/linear.py:145-157) at the bars of tests/test_gpu_tile_rows.py.  The smallest shapes at
which it can go wrong: one tile with 16 k-steps (the fewest that defer), 17 .. 20 k-steps (every exit of the loop unrolled by the ring
size), a second, ragged row tile, a ragged column tile (narrow stores), ranks 16 (the second slice of the side product stashed as
zeros) and 32, bias, every output type.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import lqer_oracle as O  # the checker

DEV = "cuda:0"


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import lqer_amd

    return lqer_amd


CASES = [  # M, K, N, rank, bias, dtype
    (128, 1024, 256, 32, False, torch.float16),   # one tile, 16 k-steps: no step behind the deferred ones
    (128, 1024, 256, 16, True, torch.bfloat16),
    (128, 1088, 256, 32, True, torch.float32),    # 17 k-steps: the loop's first exit; fp32: the accumulator's own bits
    (128, 1152, 256, 16, False, torch.float16),   # 18
    (128, 1216, 256, 32, False, torch.bfloat16),  # 19
    (128, 1280, 256, 16, True, torch.float32),    # 20: a whole trip
    (130, 1024, 256, 32, True, torch.float16),    # a second row tile with two live rows
    (128, 1024, 272, 32, False, torch.bfloat16),  # a second column tile with 16 live columns: narrow stores
    (130, 1088, 272, 16, False, torch.float32),
    (130, 1280, 272, 32, True, torch.float16),
]


def _pins():
    from lqer_amd import _lib

    return _lib.TUNE_TILE_ROWS_128, _lib.TUNE_TILE_ROWS_128 | _lib.TUNE_NO_KSPLIT


@functools.lru_cache(maxsize=None)
def _case(M, K, N, r, bias, dtype):
    """The module on the device, its input, and the oracle's answer (computed once per shape)."""
    import lqer_amd
    from bench import MXINT_Q, make_case

    case = make_case(M, K, N, max(r, 16), seed=53, bias=bias)
    x, W, A, B = case[:4]
    A, B = A[:, :r].contiguous(), B[:r].contiguous()
    mod = lqer_amd.LinearFlexibleLqer(K, N, bias=bias, q_config=MXINT_Q, l_config={"rank": r})
    sd = {"weight": W, "A": A, "B": B}
    if bias:
        sd["bias"] = case[4]
    mod.load_state_dict(sd)
    mod = mod.to(DEV).to(dtype)
    h = lambda t: None if t is None else t.to(dtype).float()
    ref = O.lqer_linear_forward(h(x), h(W), h(case[4]) if bias else None, h(A), h(B), MXINT_Q)
    return mod, x.to(dtype).to(DEV), ref


def _on_tile_route(mod, M, dtype):
    import ctypes as C

    from lqer_amd import _lib

    d = mod._desc()
    dtc = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16, torch.float32: _lib.F32}[dtype]
    return _lib.lib().lqer_gemm_route(C.byref(d), M, dtc) == _lib.ROUTE_TILE128 and _lib.lib().lqer_gemm_tile_rows(C.byref(d), M, dtc) == 128


@pytest.mark.parametrize("M,K,N,r,bias,dtype", CASES)
def test_k_split_equals_the_kernel_it_replaces_and_the_oracle(lq, M, K, N, r, bias, dtype):
    new, old = _pins()
    mod, xd, ref = _case(M, K, N, r, bias, dtype)
    try:
        mod.tuning = new
        assert _on_tile_route(mod, M, dtype)
        y_new = mod(xd).clone()
        mod.tuning = old
        y_old = mod(xd).clone()
    finally:
        mod.tuning = 0
    err = float((y_new.float().cpu() - ref).norm() / ref.norm())
    print(f"k split {M}x{K}x{N} r{r} {dtype}: rel-L2 vs oracle {err:.3e}, max |new - old| {float((y_new.float() - y_old.float()).abs().max()):.3e}")
    assert torch.equal(y_new, y_old)
    assert err <= (4e-3 if dtype == torch.bfloat16 else 1e-3), err


def test_k_split_under_graph_replay(lq):
    new, _ = _pins()
    M, K, N, r, bias, dtype = CASES[-1]
    mod, xd, _ = _case(M, K, N, r, bias, dtype)
    try:
        mod.tuning = new
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
    finally:
        mod.tuning = 0
    assert torch.equal(y1, y0)


def test_k_split_on_two_streams(lq):
    """Forwards issued alternately on two streams (each module copy with its own workspace) give the bits of the forwards alone."""
    import copy

    new, _ = _pins()
    M, K, N, r, bias, dtype = CASES[-1]
    mod, xd, _ = _case(M, K, N, r, bias, dtype)
    xs = [xd, (xd * 0.5).contiguous()]
    mods = [mod, copy.deepcopy(mod)]
    try:
        for m in mods:
            m.tuning = new
        ref = [mods[i](xs[i]).clone() for i in (0, 1)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
        outs = [[], []]
        for _ in range(12):
            for i in (0, 1):
                with torch.cuda.stream(streams[i]):
                    outs[i].append(mods[i](xs[i]))
        torch.cuda.synchronize()
    finally:
        mod.tuning = 0
    for i in (0, 1):
        for y in outs[i]:
            assert torch.equal(y, ref[i])

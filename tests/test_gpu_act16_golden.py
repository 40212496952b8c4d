"""The one-launch block-16 activation kernel (lqer_amd/csrc/act16_fused.hip) against recorded outputs of the kernel it replaced
(tests/golden/act16_fused_*.npz, written by tests/golden/make_golden_act16.py on the parent commit): the activation image - rows past M
and k past K included - and xAq bit for bit, for the shapes at which the kernel takes another path (one slab and seven idle waves, a
part-filled slab, one slab per wave, a second slab on wave 0), both 16-bit dtypes, ranks 16 / 32 / 64; inputs with all-zero blocks,
blocks at extreme exponents (the quantizer's element routine) and an outlier channel; and a captured graph replayed twice.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _act16_cases as A  # noqa: E402


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import lqer_amd

    return lqer_amd


@functools.lru_cache(maxsize=None)
def _golden(M, K):
    with np.load(A.golden_path(M, K)) as z:
        return {k: z[k] for k in z.files}


def _side(lq, M, K, r, name):
    g = _golden(M, K)
    assert np.array_equal(g["x"], A.make_x16(M, K)), "the recorded tokens are not what make_x16 builds"
    side = A.ActSide(A.make_module(lq, K, r, A.DTYPES[name]), A.x_for(g["x"], name).to(A.DEV))
    assert A.crc(side.p["a_t_b16"]) == int(g[f"crc_a_{name}_r{r}"][0]), "the A^T image differs from the recorded run's"
    return side, g


def _check(side, g, name, r):
    img, xa = side.read()
    assert np.array_equal(img, g[f"img_{name}"])
    assert np.array_equal(xa, g[f"xaq_{name}_r{r}"])


@pytest.mark.parametrize("name", list(A.DTYPES))
@pytest.mark.parametrize("r", A.RANKS)
@pytest.mark.parametrize("M,K", A.SHAPES)
def test_image_and_xaq_bit_for_bit(lq, M, K, r, name):
    side, g = _side(lq, M, K, r, name)
    side.launch()
    _check(side, g, name, r)


def test_graph_replay_same_bits(lq):
    M, K, r, name = 24, 4096, 32, "f16"
    side, g = _side(lq, M, K, r, name)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side.launch()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        side.launch()
    for _ in range(2):
        side.ws.fill_(0x5A)
        graph.replay()
        _check(side, g, name, r)

"""The fused GEMM's 128-row tile kernel (lqer_amd/csrc/gemm_w4a8.hip) against recorded outputs of the parent of the commit that changed
its main loop's weight expand (tests/golden/gemm128_*.npz, written by tests/golden/make_golden_gemm128.py): y bit for bit, for the
shapes, ranks, B_out modes and tensor types of tests/_gemm128_cases.py.  The weight images hold all 16 nibble codes (-0 planted: the
packer never writes it) and at least four binades of block exponents; two cases hold exponent bytes beyond the table-free expand and
must take the table form.
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm128_cases as G  # noqa: E402


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import lqer_amd

    return lqer_amd


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_y_bit_for_bit(lq, case):
    with np.load(G.golden_path(case)) as z:
        want, seed, crcs = z["y"], int(z["seed"][0]), z["crc_inputs"]
    assert seed == G.seed_of(case)
    inputs = G.make_inputs(case)
    assert np.array_equal(G.input_crcs(inputs), crcs), "the inputs are not the recorded run's"
    bits, (planted, codes, ebytes) = G.run_case(lq, case, inputs)
    assert planted > 0 and len(codes) == 16, (planted, codes)
    assert len(ebytes) >= 4, ebytes
    assert (int(ebytes.max()) > 245) == (case[7] == "huge"), ebytes
    assert bits.shape == want.shape and bits.dtype == want.dtype
    bad = np.argwhere(bits != want)
    assert bad.size == 0, f"{len(bad)} of {bits.size} elements differ, first at {bad[0]}: {bits[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def test_an_image_beyond_the_table_free_expand_asks_for_the_table(lq):
    """lqer_f16_prepare's flags[0] & 2 (ops.w_exp_needs_table) is raised exactly from exponent byte 246 on."""
    from bench import MXINT_Q
    from lqer_amd import ops

    fmt = ops.make_qfmt(MXINT_Q["w_quantizer"], "w")
    for top, want in ((2.0 ** 121, False), (1.25 * 2.0 ** 121, True)):  # block exponents 121 / 122: bytes 245 / 246
        W = torch.full((16, 64), 0.01)
        W[5, 17] = top
        img = ops.pack_weight(W.to(G.DEV), fmt)
        assert int(img.view(-1, 576)[:, 512:].max()) == (246 if want else 245)
        assert ops.w_exp_needs_table(img, 16, 64, fmt) is want

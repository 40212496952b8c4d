"""Every GEMM route of the Linear forward, bit for bit, over every output element, rooted in the oracle.

tests/test_gpu_gemm256_exact.py does this for the main product of the 256-row tile kernel; the other routes are compared with the
oracle by a relative L2 norm over the whole output, which cannot see a local error (one element 20 % off, a wrong 16-column tail, a
B_out block with its exponent one too high, a tie rounded the wrong way).  Here the WHOLE forward - main product, side path, bias - runs
on the operands of tests/_exact_cases.py, whose fp32 partial sums are exact in any order (asserted per case before anything is
compared, and without a GPU by tests/test_exact_cases_cpu.py), so that y must equal round_to_dtype(float64 value) at every element,
whatever the summation order, k-split, limb split or expand of the kernel that ran:

  one-launch decode (decode1.hip) and its group launch; the compact 2- / 3-bit image readers; the small-M weight-streaming kernel at
  1 .. 4 token tiles; 64-row tiles; the prologue / deferred / k-split / staged / table-expand / pre-pass instantiations of the 128-row
  tile kernel; the int8 kernel at both tile heights, weight blocks of 128, one per row and the image of 8-bit codes, with every way the
  B_out row maxima travel; the fp16 pass-through main loop; one whole forward on 256-row tiles.

Every case asserts what the packing chose for x, the route, the tile rows and the decode-partials answer before it runs ONCE, and
prints one line: kernel, route, rows, pins, bounds, count of differing elements.  On a failure it prints the first differing (row,
column, got, want) and the counts per 16-column block and per row tile, so that the failing lane group can be read off.  The only
tolerance is equality.  A differing element is a kernel or host bug by construction: the oracle's value does not depend on order.

Left out: the A16 side path - its pass-through A_out carries x A as two bf16 limbs, and keeping x A within 16 bits needs a separate
fixture.  A16_Q runs with rank 0 (the fp16 main loop).
Run on the GPU box:  python -m pytest tests -m gpu -x -q"""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_cases as E  # noqa: E402

DEV = E.DEV


@pytest.fixture(scope="module")
def lq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import lqer_amd

    return lqer_amd


def _report(tag, y, want, tile_rows):
    """Count of differing elements; on a difference, where: the first one and the counts per 16-column block and per row tile."""
    bad = y != want
    ndiff = int(bad.sum())
    if ndiff:
        r, c = [int(v) for v in bad.nonzero()[0]]
        per_block = [int(bad[:, j:j + 16].sum()) for j in range(0, bad.shape[1], 16)]
        tr = tile_rows or 16
        per_tile = [int(bad[i:i + tr].sum()) for i in range(0, bad.shape[0], tr)]
        print(f"{tag}: first differing element (row {r}, column {c}): got {float(y[r, c])!r} want {float(want[r, c])!r}; "
              f"per 16-column block {per_block}; per {tr}-row tile {per_tile}")
    return ndiff


def _device_module(fx, dtype, image="standard", flags=None, tuning=0):
    mod = E.make_module(fx, image=image, flags=flags, tuning=tuning).to(DEV).to(dtype)
    mod.pack()
    return mod


@pytest.mark.parametrize("cid", [c.id for c in E.CASES])
def test_forward_equals_the_oracle_at_every_element(lq, cid):
    from lqer_amd import _lib, ops

    c = E.BY_ID[cid]
    fx, dtype = c.fx, E.DTYPES[c.dtype]
    f = E.fixture(fx)
    # the condition of the comparison, asserted (never a reason to skip): every partial sum of every stage is exact in fp32 in any order
    for stage, bound in f["bounds"].items():
        assert bound < 1.0, (stage, bound)
    mod = _device_module(fx, dtype, c.image, c.flags, E.tuning_bits(c))
    # what the packing decided for x, then the plan's answers for the very descriptor the forward uses
    assert ("i8" if mod._x_i8 else "f16" if mod._x_f16 else "mx") == c.x_kind
    assert not mod._w_exp_table or "W_EXP_TABLE" in c.tune
    desc = mod._desc()
    route, rows, partials = E.plan_answers(desc, fx.M, c.dtype)
    assert (route, rows, partials) == (c.route, c.rows, c.partials), (route, rows, partials)
    xd = f["x"].to(dtype).to(DEV)
    assert torch.equal(xd.float().cpu(), f["x"])
    if c.image == "narrow":  # the compact image is read directly, in one launch up to 8 tokens
        p = mod._packed
        nr = _lib.lib().lqer_weight_narrow_route(C.byref(desc), fx.M, ops.dtype_code(xd), fx.K, int(p.get("a_limbs", 0)), int(p.get("b_limbs", 0)))
        assert nr == (_lib.NARROW_DIRECT_ONE_LAUNCH if fx.M <= 8 else _lib.NARROW_DIRECT), nr
    y = mod(xd)
    torch.cuda.synchronize()
    want = f["y64"].to(dtype)  # the one rounding
    assert y.shape == want.shape and y.dtype == dtype
    ndiff = _report(cid, y.cpu(), want, rows)
    print(f"exact {c.kernel} {fx.cfg} {fx.M}x{fx.K}x{fx.N} r{fx.r}{' bias' if fx.bias else ''} {c.dtype}: route {route} rows {rows} "
          f"pins [{' '.join(c.tune)}] image {c.image} bounds {E.bounds_text(f)} differing {ndiff}")
    assert torch.equal(y.cpu(), want)
    if fx.bias:  # like the reference, the parameter now holds b_quantizer(bias): the term that was added
        assert torch.equal(mod.bias.detach().float().cpu(), f["out"]["bq"])


def test_group_launch_gives_each_member_its_own_oracle_value(lq):
    """lqer_linear_forward_group: three Linears handed the same 3 tokens in ONE launch (the producers multiply x with the concatenated A),
    N = 272 / 144 / 272, the last one with a bias - each member's output against its own oracle value, every element."""
    from lqer_amd.linear import SharedActivation

    dtype = E.DTYPES[E.GROUP_DTYPE]
    fs = [E.fixture(fx) for fx in E.GROUP]
    for f in fs:
        for stage, bound in f["bounds"].items():
            assert bound < 1.0, (stage, bound)
    mods = [_device_module(fx, dtype) for fx in E.GROUP]
    grp = SharedActivation(mods)
    assert grp.enabled
    xd = fs[0]["x"].to(dtype).to(DEV)
    ys = [mods[0](xd)]
    assert grp._dys is not None and len(grp._dys) == 3  # the group launch ran: the other members are handed its outputs
    ys += [m(xd) for m in mods[1:]]
    torch.cuda.synchronize()
    assert grp._dys is None  # (every member served from the one launch)
    total = 0
    for fx, f, y in zip(E.GROUP, fs, ys):
        want = f["y64"].to(dtype)
        nd = _report("group " + E.fx_id(fx), y.cpu(), want, 0)
        print(f"exact group member {E.fx_id(fx)} {E.GROUP_DTYPE}: bounds {E.bounds_text(f)} differing {nd}")
        total += nd
    assert total == 0
    for fx, f, y in zip(E.GROUP, fs, ys):
        assert torch.equal(y.cpu(), f["y64"].to(dtype))

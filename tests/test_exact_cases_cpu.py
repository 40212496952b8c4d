"""The fixtures and the case table of tests/test_gpu_exact_routes.py, checked without a GPU (tests/_exact_cases.py): for EVERY fixture the
three exactness bounds are below 1, the oracle's fp32 stages equal their float64 values (so the oracle's y does not depend on the
order of any sum), the inputs are the recorded PCG64 draws, the re-quantizers meet exact ties, every 16-column block has live output;
for every case the route, tile rows and decode-partials answer of the library's host-only plan calls are the ones the case claims, so
that the GPU test cannot silently run another kernel.  Nothing here is a reason to skip: each property is asserted."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_cases as E  # noqa: E402

# crc32 over the operand bytes of every fixture (numpy PCG64 seeded by the fixture's id): the inputs do not drift with a library version
CHECKSUMS = {
    "mx-m8-k320-n272-r32": 0x1015d138, "mx-m1-k320-n272-r32": 0x2d343dee, "mx-m8-k1088-n272-r32": 0x5cd2252d,
    "mx-m8-k1088-n264-r16": 0xe353df4b, "mx-m1-k1088-n260-r48": 0xc04898c0, "mx-m8-k320-n260-r48": 0x6ada2e95,
    "mx_pass-m8-k1088-n272-r32": 0x4236217, "mx_pass-m1-k320-n264-r16": 0x4907f59c, "opt-m8-k320-n272-r32-bias": 0x95464743,
    "opt-m1-k1088-n264-r16-bias": 0xa1422344, "mx-m8-k320-n272-r0": 0x1d175005, "mx-m1-k1088-n260-r0": 0xe6951544,
    "w2b32-m8-k320-n272-r32": 0xc184199e, "w2b32-m20-k320-n272-r32": 0x8235b626, "w3b16-m8-k320-n272-r32": 0x91dea259,
    "w3b16-m20-k320-n272-r32": 0x7d3b6a84, "mx-m9-k320-n272-r32": 0x7a4d2960, "mx-m16-k1088-n264-r32": 0xbff3d618,
    "mx-m17-k320-n260-r0": 0x9f2a1ac4, "mx-m33-k1088-n272-r32": 0x1084b3, "mx-m33-k320-n272-r0": 0xc28c17c4,
    "mx_pass-m48-k320-n264-r32": 0xc144a8ac, "mx-m49-k1088-n260-r32": 0xa393d0a8, "mx-m64-k320-n272-r32": 0x6c3a038,
    "mx-m64-k1088-n272-r0": 0x79668395, "mx_pass-m64-k1088-n260-r32": 0x6acad98e, "mx-m130-k320-n272-r32": 0x93839576,
    "mx-m65-k1024-n264-r32": 0xf2fa4e7d, "mx-m65-k320-n260-r0": 0xde801e95, "mx-m130-k1024-n272-r0": 0xd647edb9,
    "opt-m130-k1024-n272-r32-bias": 0x68eadcd9, "mx_pass-m130-k320-n260-r32": 0xff578bbe, "mx-m128-k320-n264-r0": 0xce23bf6a,
    "mx-m130-k320-n260-r48": 0x1978f015, "mx-m130-k1024-n272-r32": 0x71ad4e42, "mx-m130-k1088-n272-r32": 0x1b7a4cb7,
    "mx-m128-k1024-n260-r8": 0x2c658f4f, "mx-m130-k1024-n272-r48": 0x19a97660, "mx_pass-m130-k1024-n272-r32": 0x97971974,
    "mx_row-m130-k320-n272-r32": 0x99fb2746, "mx_row-m128-k1024-n264-r32": 0x5a57625a, "mx_row-m7-k320-n272-r32": 0x9aaad865,
    "int-m130-k384-n272-r32": 0xfe4cc67e, "int-m130-k1024-n272-r0": 0x18edaa57, "int-m258-k1024-n272-r64": 0x5c53ff36,
    "introw-m130-k1024-n264-r32": 0xfbe11219, "w8a8-m130-k384-n272-r32": 0xd1de6124, "int-m258-k384-n264-r0": 0xca925968,
    "introw-m258-k384-n260-r32": 0xe20bd20, "w8a8-m258-k1024-n272-r64": 0xb5f8e305, "w8a8-m258-k384-n272-r0": 0x4d4ab2b4,
    "a16-m8-k320-n272-r0": 0xb82da182, "a16-m130-k320-n272-r0": 0x298b3c8b, "mx-m4098-k320-n2276-r32-bias": 0xbd682662,
    "mx-m3-k320-n272-r32": 0xd35d6883, "mx-m3-k320-n144-r32": 0x481fc781, "opt-m3-k320-n272-r32-bias": 0xfa98957e,
}


@pytest.fixture(scope="module")
def lib():
    from lqer_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_every_fixture_has_a_checksum_and_every_case_a_fixture():
    assert sorted(CHECKSUMS) == sorted(E.fx_id(fx) for fx in E.FIXTURES)
    assert len({E.fx_id(fx) for fx in E.FIXTURES}) == len(E.FIXTURES)
    assert all(c.fx in E.FIXTURES for c in E.CASES)


@pytest.mark.parametrize("fx", E.FIXTURES, ids=E.fx_id)
def test_fixture_is_exact_in_any_order(fx):
    f = E.fixture(fx)
    print(f"exact fixture {E.fx_id(fx)}: bounds {E.bounds_text(f)} units " + " ".join(f"{k} 2^{int(torch.log2(torch.tensor(v)))}" for k, v in f["units"].items())
          + f" ties {f['ties']}")
    assert E.checksum(fx) == CHECKSUMS[E.fx_id(fx)]
    for t in (f["x"], f["W"], f["A"], f["B"], f["b"]):  # exact in every element type the cases run
        assert t is None or (torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t))
    # the condition of every comparison: the magnitudes of a stage's terms add up to less than 2^24 grid units
    for stage, bound in f["bounds"].items():
        assert bound < 1.0, (stage, bound)
    out = f["out"]
    if fx.r > 0:
        assert torch.equal(out["xA"].double(), f["xA64"])
        assert torch.equal(out["xAB"].double(), f["xAB64"])
    assert torch.equal(out["y"].double(), f["y64"])
    # ... and every partial sum lies on its stage's grid: the float64 values are whole multiples of the unit
    for stage, v in (("xA", f.get("xA64")), ("xAB", f.get("xAB64")), ("y", f["y64"])):
        if v is not None:
            q = v / f["units"][stage]
            assert torch.equal(q, q.round()), stage
    # the features the fixtures keep: an outlier channel, a zero block, a zero weight row at the last live column, a zero x block in
    # the last row; from 8 rows a zero row
    x, W = f["x"], f["W"]
    assert (fx.M < 8 or float(x[:, 7].abs().max()) > 8.0) and not bool(W[fx.N - 1].any()) and not bool(W[2, 16:32].any())
    assert not bool(x[min(1, fx.M - 1), 32:48].any()) and (fx.M < 3 or not bool(x[fx.M - 1, :16].any())) and (fx.M < 8 or not bool(x[5].any()))
    nb = (fx.N + 15) // 16
    if fx.r > 0:
        # live output in every 16-column block - of the side path's own term too
        for name, v in (("y", f["y64"]), ("xABq", out["xABq"])):
            live = [bool(v[:, j * 16:(j + 1) * 16].ne(0).any()) for j in range(nb)]
            assert all(live), (name, live)
        qb = f["qs"]["B_out"]
        if qb["name"] == "block_fp":
            _, exps, L = E._block_exps(f["xAB64"], qb)
            if exps.shape[1] > 1:  # several B_out blocks per row: at least one whose exponent differs from its neighbour's
                assert bool((exps[:, 1:] != exps[:, :-1]).any())
        if fx.M >= 64:  # exact ties in front of both re-quantizers
            assert f["ties"]["A_out"] >= 1, f["ties"]
            assert qb["name"] != "block_fp" or f["ties"]["B_out"] >= 1, f["ties"]
    else:
        assert all(bool(f["y64"][:, j * 16:min((j + 1) * 16, fx.N - 1)].ne(0).any()) for j in range(nb) if j * 16 < fx.N - 1)


def test_decode_size_fixtures_meet_ties_taken_together():
    dec = [E.fixture(fx) for fx in E.FIXTURES if fx.r > 0 and fx.M < 64]
    assert len(dec) >= 10
    assert sum(f["ties"]["A_out"] for f in dec) >= 1 and sum(f["ties"]["B_out"] for f in dec) >= 1


def test_the_group_members_share_their_tokens():
    xs = [E.fixture(fx)["x"] for fx in E.GROUP]
    assert all(torch.equal(x, xs[0]) for x in xs[1:])
    assert [fx.N for fx in E.GROUP] == [272, 144, 272]


@pytest.mark.parametrize("cid", [c.id for c in E.CASES])
def test_case_runs_the_kernel_it_claims(lib, cid):
    c = E.BY_ID[cid]
    got = E.plan_answers(E.host_desc(c), c.fx.M, c.dtype)
    assert got == (c.route, c.rows, c.partials), f"{cid}: the library says {got}"
    if c.kernel.startswith("decode1"):  # the one-launch kernel's own limits (csrc/common.h, d1::): 8 token rows, K in whole blocks of 16
        assert c.fx.M <= 8 and c.fx.K % 16 == 0 and c.partials == 1
    if c.kernel.startswith("smallm-mt"):  # 16-row token tiles of the small-M kernel
        assert (4 if c.fx.M > 48 else (c.fx.M + 15) // 16) == int(c.kernel[len("smallm-mt")])


def test_the_table_reaches_every_piece():
    kernels = {c.kernel for c in E.CASES}
    for want in ("decode1", "decode1-narrow", "smallm-narrow-mt2", "smallm-mt1", "smallm-mt2", "smallm-mt3", "smallm-mt4", "tile64",
                 "tile128-prologue", "tile128-defer", "tile128-defer-ksplit", "tile128-defer-staged", "tile128-prologue-staged",
                 "tile128-defer-ksplit-table", "tile128-bout-pass", "tile128-bout-row", "tile128-bout-row-decode", "i8-128", "i8-256",
                 "i8-128-codes", "i8-256-codes", "smallm-f16x", "tile64-f16x", "tile256"):
        assert want in kernels, want
    for k in ("decode1", "tile64", "tile128-defer-ksplit"):  # the three element types on the kernels every step runs
        assert {c.dtype for c in E.CASES if c.kernel == k} == {"f16", "bf16", "f32"}, k
    assert {c.fx.N % 16 for c in E.CASES} >= {0, 8, 4}  # N = 272, 264 (odd multiple of 8), 260 (N % 8 != 0)

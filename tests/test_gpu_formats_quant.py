"""Narrow block_fp formats (exponent clamps at both ends, every width) through the standalone quantizer and packing kernels,
bit for bit against the oracle.  The formats, the (format, width) pairs and the input ladder are tests/_formats.py; the oracle is
pinned on them by tests/golden/quantizers_expfield.npz (tests/test_oracle_golden.py).  Every test asserts on the CPU, before its
first GPU call, that the oracle itself clamps at least 15 % of the non-zero blocks at each end the dtype can reach.

No tolerance anywhere in this module: quantization is deterministic, every comparison is torch.equal.

The C ABI has no call that asks for the bf16 image together with `deq`: the image-alone fast route (quantize.hip emit16, first
branch) is reached through quantize_act, the general route through quantize_mxint (deq / codes / exps), and the general route's
bf16 store through the zero blocks and the blocks outside mxint16_fast_ok of a quantize_act call.
"""
import pytest
import torch

import _formats as F
from oracle import lqer_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lqer_amd import ops as _ops

    return _ops


def _pairs_for(pairs, dt):
    return [p for p in pairs if dt != "f16" or p[0] in F.FP16_IDS]


def _cases(pairs):
    return [pytest.param(p, dt, id=f"{F.pair_id(p)}-{dt}") for dt in DTYPES for p in _pairs_for(pairs, dt)]


def _flushed(x, ref):
    """What packed and bf16 images hold: the quantizer's output with the |x| <= 1e-8 pass-through as 0."""
    return torch.where(x.float().abs() <= 1e-8, torch.zeros_like(ref), ref)


@pytest.mark.parametrize("pair,dt", _cases(F.ACT_PAIRS))
def test_quantize_mxint_deq_codes_exps(ops, pair, dt):
    """ops.quantize_mxint: blocks of 16 (k_quant_seg16), 32 (k_quant_blk) and the whole row (k_quant_row), ragged rows."""
    fid, width = pair
    dtype = DTYPES[dt]
    inputs = []
    for n, (block, rows, cols) in enumerate(((16, 12, 200), (32, 12, 200), (-1, 24, 136))):
        x = F.ladder(fid, dtype, rows, cols, block, seed=10 + n)
        c = F.cfg(fid, width, [1, block])
        F.assert_covered(x, fid, c)
        inputs.append((block, x, c))
    for block, x, c in inputs:
        ref, codes, exps = F.oracle_q(x, c, decompose=True)
        got = ops.quantize_mxint(x.to(DEV), ops.make_qfmt(c, "x"))
        assert torch.equal(got["deq"].cpu(), ref), block
        assert torch.equal(got["codes"].cpu().to(torch.int32), codes), block
        assert torch.equal(got["exps"].cpu().to(torch.int32), exps.reshape(x.shape[0], -1).clamp(-128, 127)), block
        only = ops.quantize_mxint(x.to(DEV), ops.make_qfmt(c, "x"), want=("deq",))["deq"].cpu()
        assert torch.equal(only, ref), block


@pytest.mark.parametrize("pair,dt", _cases(F.ACT_PAIRS))
def test_quantize_act_bf16_image(ops, pair, dt):
    """lqer_quantize_act_mxint: the bf16 image alone (the packed-fp32 fast route where the scale is a normal float), zero padding."""
    fid, width = pair
    dtype = DTYPES[dt]
    inputs = []
    for n, (block, M, K) in enumerate(((16, 13, 200), (32, 13, 200), (-1, 24, 136))):
        x = F.ladder(fid, dtype, M, K, block, seed=20 + n)
        c = F.cfg(fid, width, [1, block])
        F.assert_covered(x, fid, c)
        inputs.append((x, c))
    for x, c in inputs:
        M, K = x.shape
        xq = ops.quantize_act(x.to(DEV), ops.make_qfmt(c, "x")).cpu()
        assert xq.shape[0] % 256 == 0 and xq.shape[1] % 64 == 0
        assert torch.equal(xq[:M, :K].float(), _flushed(x, F.oracle_q(x, c))), c["block_size"]
        assert not xq[:M, K:].any()


@pytest.mark.parametrize("pair,dt", _cases(F.ACT_PAIRS))
def test_quantize_act_int8_image_and_row_scale(ops, pair, dt):
    """The int8 route's activation image: one exponent per token row, mantissa x row scale == the quantizer (k_quant_row8 for aligned
    16-bit rows, k_quant_row otherwise: K = 136 is a multiple of 8, K = 100 is not)."""
    fid, width = pair
    dtype = DTYPES[dt]
    inputs = []
    for n, (M, K) in enumerate(((24, 136), (24, 100))):
        x = F.ladder(fid, dtype, M, K, -1, seed=30 + n)
        c = F.cfg(fid, width, [1, -1])
        F.assert_covered(x, fid, c)
        inputs.append((x, c))
    for x, c in inputs:
        M, K = x.shape
        codes, scales = ops.quantize_act_i8(x.to(DEV), ops.make_qfmt(c, "x"))
        codes, scales = codes.cpu(), scales.cpu()
        assert torch.equal(codes[:M, :K].float() * scales[:M, None], _flushed(x, F.oracle_q(x, c))), K
        assert not codes[:M, K:].any() and int(codes.abs().max()) <= 2 ** (width - 1) - 1


def _tiled(fid, dtype, groups, R, cols, L, seed):
    """[groups * R, cols]: R consecutive rows share a ladder row's scales, so that R x L tiles meet the clamps like the ladder's blocks."""
    t = F.ladder(fid, torch.float32, groups, cols, L, seed=seed)
    jit = 0.5 + 0.5 * torch.rand(groups, R, cols, generator=torch.Generator().manual_seed(seed))
    jit[:, 0] = 1.0
    return (t[:, None, :] * jit).reshape(groups * R, cols).to(dtype)


@pytest.mark.parametrize("pair", [("e4", 8), ("e3b6", 4), ("e3bm2", 8), ("e1", 4), ("e5b20", 6)], ids=F.pair_id)
def test_quantize_act_tiles(ops, pair):
    """ops.quantize_act_tiles: [2, 16] tiles of a 3-D activation and [4, 16] tiles of a 2-D one (k_tile_amax / k_tile_quant)."""
    fid, width = pair
    x3 = _tiled(fid, torch.float32, 6, 2, 56, 16, seed=41).reshape(2, 6, 56).contiguous()
    c3 = F.cfg(fid, width, [2, 16], True)
    x2 = _tiled(fid, torch.bfloat16, 5, 4, 56, 16, seed=42)[:18].contiguous()
    c2 = F.cfg(fid, width, [4, 16], False)
    F.assert_covered(x3, fid, c3)
    F.assert_covered(x2, fid, c2)
    for x, c in ((x3, c3), (x2, c2)):
        got = ops.quantize_act_tiles(x.to(DEV), ops.make_qfmt(c, "x")).cpu()
        assert got.dtype == x.dtype and torch.equal(got.float(), F.oracle_q(x, c)), c["block_size"]


def _weight_inputs(fid, width, dtype):
    """(x, config) for blocks of 16 / 128 / the whole row (ragged K) and 2-D tiles [4, 16]; N <= 48, K <= 320."""
    out = []
    for n, (block, N, K) in enumerate(((16, 40, 200), (128, 24, 320), (-1, 48, 72))):
        out.append((F.ladder(fid, dtype, N, K, block, seed=50 + n), F.cfg(fid, width, [1, block], False)))
    out.append((_tiled(fid, dtype, 11, 4, 72, 16, seed=53)[:42].contiguous(), F.cfg(fid, width, [4, 16], False)))
    for x, c in out:
        F.assert_covered(x, fid, c)
    return out


@pytest.mark.parametrize("pair,dt", [pytest.param(p, dt, id=f"{F.pair_id(p)}-{dt}") for dt in ("f32", "bf16") for p in F.W4_PAIRS + F.W8_PAIRS])
def test_pack_unpack_weight(ops, pair, dt):
    """pack_weight -> unpack_weight == the oracle with the declared |w| <= 1e-8 flush: the 4-bit image (widths 2, 3, 4) and the three
    limbs (5, 6, 8)."""
    fid, width = pair
    for x, c in _weight_inputs(fid, width, DTYPES[dt]):
        fmt = ops.make_qfmt(c, "w")
        N, K = x.shape
        w = ops.unpack_weight(ops.pack_weight(x.to(DEV), fmt), N, K, fmt).cpu()
        assert torch.equal(w, _flushed(x, F.oracle_q(x, c))), c["block_size"]


def _i8_eligible(x, c):
    """lqer_i8_prepare's decision, restated from the oracle's codes and exponents (N <= 256: one tile of rows).  Per row, the
    exponent bytes e - mbits + 127 of its groups of 128 k that hold a non-zero code.  An image of 5..8-bit codes takes one byte per
    row.  The 4-bit image: rows that spread their bytes over at most 4 carry the shift in the int8 lane (code << 4 - (max - byte)),
    otherwise - decided for the tile - the main loop folds (16 code << byte - min, at most 20); either way the largest sum a row
    can reach against 127 stays below 2^31, and the row's scale is a normal float.
    The thresholds (4, 20, the byte floors 2 and 5, 2^31) are the kernel's own, transcribed: this pins today's decision on the oracle's
    data - a refusal or an acceptance that changes is seen - and does not derive it independently.  What is independent are the two
    unconditional assertions of the test: a whole-row block is always accepted, and so is a 4-bit image whose range spans at most 7."""
    width = c["width"]
    mbits = width - 1
    _, codes, exps = F.oracle_q(x, c, decompose=True)
    N, K = x.shape
    L = K if c["block_size"][1] == -1 else c["block_size"][1]
    exps = exps.reshape(N, -1)
    rows = []
    for n in range(N):
        row = []
        for k0 in range(0, K, 128):
            a = int(codes[n, k0:k0 + 128].abs().sum())
            es = {int(exps[n, k // L]) for k in range(k0, min(k0 + 128, K)) if int(codes[n, k]) != 0}
            if len(es) > 1:
                return False
            if a:
                row.append((min(max(es.pop() - mbits + 127, 1), 254), a))
        rows.append(row)
    spread = [max(b for b, _ in r) - min(b for b, _ in r) for r in rows if r]
    if width > 4:
        return all(s == 0 for s in spread) and all(sum(a for _, a in r) * 127 < 2 ** 31 and r[0][0] >= 2 for r in rows if r)
    preshift = any(s > 0 for s in spread) and not any(s > 4 for s in spread)
    for r in rows:
        if not r:
            continue
        bmin, bmax = min(b for b, _ in r), max(b for b, _ in r)
        if preshift:
            bound = sum((a << (4 - (bmax - b))) * 127 for b, a in r)
        else:
            if bmax - bmin > 20:
                return False
            bound = sum((a << (b - bmin)) * 16 * 127 for b, a in r)
        if bound >= 2 ** 31 or (bmax if preshift else bmin) < 5:
            return False
    return True


@pytest.mark.parametrize("pair", F.W4_PAIRS + F.W8_PAIRS, ids=F.pair_id)
def test_int8_weight_image(ops, pair):
    """lqer_i8_prepare's image of codes (blocks of 128 and whole rows), read back: the oracle's quantizer.  A row whose group exponents
    span more than the i32 accumulator allows is refused (ok False), and so is an 8-bit code image with more than one exponent per row -
    never one exponent per row, and never a 4-bit image whose whole exponent range spans at most 7.  The decision itself must be the one
    _i8_eligible works out from the oracle, so that neither a wrong refusal nor a wrong acceptance passes."""
    fid, width = pair
    emin, emax = F.e_range(fid)
    inputs = []
    for n, (block, N, K) in enumerate(((128, 24, 320), (-1, 48, 200))):
        x = F.ladder(fid, torch.float32, N, K, block, seed=60 + n)
        c = F.cfg(fid, width, [1, block], False)
        F.assert_covered(x, fid, c)
        inputs.append((block, x, c))
    for block, x, c in inputs:
        fmt = ops.make_qfmt(c, "w")
        N, K = x.shape
        packed = ops.pack_weight(x.to(DEV), fmt)
        ok, buf = ops.i8_prepare(packed, N, K, fmt)
        if block == -1 or (width <= 4 and emax - emin <= 7):
            assert ok, (block, fid)
        assert ok == _i8_eligible(x, c), (block, fid, width)
        if ok:
            got = ops.unpack_weight_i8(buf, N, K, fmt if width > 4 else None).cpu()
            assert torch.equal(got, _flushed(x, F.oracle_q(x, c))), block


@pytest.mark.parametrize("fid,ew,bias", [(f, F.FORMATS[f][0], F.bias_of(f)) for f in F.FORMATS] + [("e3b-20", 3, -20), ("e3b30", 3, 30)])
def test_f16_eligibility_follows_the_clamped_scales(ops, fid, ew, bias):
    """lqer_f16_prepare's flag: raised exactly when some 16-k segment's scale byte e - mbits + 127 leaves [103, 140] - with a narrow
    field that is decided by the CLAMPED exponent (a field of [20, 27] is never eligible however small the weights are, one of
    [-6, 1] always is however large)."""
    width, N, K = 4, 32, 192
    base = fid if fid in F.FORMATS else "e4"
    x = F.ladder(base, torch.float32, N, K, 16, seed=70)
    c = dict(name="block_fp", width=width, exponent_width=ew, exponent_bias=bias, block_size=[1, 16], skip_first_dim=False)
    if fid in F.FORMATS:
        F.assert_covered(x, fid, c)
    _, _, exps = F.oracle_q(x, c, decompose=True)
    byte = (exps.reshape(N, -1) - (width - 1) + 127).clamp(1, 254)  # (a zero block carries exponent 0, as the padding does)
    want = bool(((byte >= 103) & (byte <= 140)).all())
    fmt = ops.make_qfmt(c, "w")
    ok, _ = ops.f16_prepare(ops.pack_weight(x.to(DEV), fmt), N, K, None, 0, 0)
    assert ok == want, (fid, int(byte.min()), int(byte.max()))
    if fid in ("e3b-20", "e3b30"):
        assert not want
    if fid in ("e3b6", "e1", "e2", "e4"):
        assert want


@pytest.mark.parametrize("pair,dt", _cases(F.ACT_PAIRS))
def test_pack_bias(ops, pair, dt):
    """lqer_pack_bias: bias_q == the oracle (the pass-through of |b| <= 1e-8 kept, zero padding) for blocks of 16 and one block."""
    fid, width = pair
    dtype = DTYPES[dt]
    b16 = F.ladder(fid, dtype, 1, 280, 16, seed=80)[0].contiguous()
    c16 = F.cfg(fid, width, [16], False)
    ball = F.ladder(fid, dtype, 9, 50, -1, seed=81)  # nine biases of one block each
    call = F.cfg(fid, width, [-1], False)
    F.assert_covered(b16, fid, c16)
    F.assert_covered(ball, fid, F.cfg(fid, width, [1, -1], True))
    got = ops.pack_bias(b16.to(DEV), ops.make_qfmt(c16, "b")).cpu()
    assert torch.equal(got[:280], F.oracle_q(b16, c16)) and not got[280:].any()
    for i in range(ball.shape[0]):
        got = ops.pack_bias(ball[i].contiguous().to(DEV), ops.make_qfmt(call, "b")).cpu()
        assert torch.equal(got[:50], F.oracle_q(ball[i], call)) and not got[50:].any(), i

"""Narrow block_fp formats for the tests: the exponent-field table, the (format, width) pairs, an input ladder that reaches
both exponent clamps, and the condition every test checks on the oracle before its first GPU call.  CPU only.

A block_fp format clamps its shared exponent to [emin, emax] = [-bias, 2^exponent_width - 1 - bias] (block_fp.py:46-51; the
default bias is 2^(exponent_width-1) - 1).  With the templates' 8-bit field nothing below 2^127 ever meets a clamp; the formats
here meet both inside what fp32 / bf16 (and, for some, fp16) hold.

The ladder: every block of `block` consecutive elements of a row gets a target exponent k, its largest magnitude lies in
(2^(k-1), 2^k], so the unclamped shared exponent is k.  One third of the blocks takes k in [emin - 4, emin - 1] (clamped from
below), one third k in [emin, emax], one third k in [emax + 1, emax + 4] (clamped from above) - each range cut to what the dtype
holds, a class that the dtype cannot reach is left out.  Added on top: one all-zero block, scattered zeros, block maxima at a
power of two and one ulp (of the dtype) to either side, and for fp32 / bf16 one |x| <= 1e-8 element in an ordinary block.
"""
from __future__ import annotations

import torch

from oracle import lqer_oracle as O

# id -> (exponent_width, exponent_bias)
FORMATS = {
    "e8": (8, None),      # [-127, 128]  control
    "e4": (4, None),      # [-7, 8]      both clamps reachable in fp16
    "e2": (2, None),      # [-1, 2]
    "e1": (1, None),      # [0, 1]       two exponents
    "e3b6": (3, 6),       # [-6, 1]      P-like range
    "e3bm2": (3, -2),     # [2, 9]       emin > 0
    "e5b20": (5, 20),     # [-20, 11]    asymmetric
    "e8b120": (8, 120),   # [-120, 135]  emax beyond any fp32 exponent, exponent bytes up to 248
}
FP16_IDS = ("e4", "e2", "e1", "e3b6", "e3bm2")  # the formats whose clamps lie inside 2^-14 .. 2^15

# every id with width 8 and with width 4; every width with e8 and with e4
ACT_PAIRS = [(i, w) for i in FORMATS for w in (8, 4)] + [(i, w) for i in ("e8", "e4") for w in (2, 3, 6)]
W4_PAIRS = [(i, 4) for i in FORMATS] + [(i, w) for i in ("e8", "e4") for w in (2, 3)]          # the 4-bit weight image
W8_PAIRS = [(i, 8) for i in FORMATS] + [(i, w) for i in ("e8", "e4") for w in (5, 6)]          # three limbs / int8 codes


def pair_id(p) -> str:
    return f"{p[0]}-w{p[1]}"


def bias_of(fid: str) -> int:
    ew, b = FORMATS[fid]
    return 2 ** (ew - 1) - 1 if b is None else b


def e_range(fid: str):
    ew, _ = FORMATS[fid]
    b = bias_of(fid)
    return -b, 2 ** ew - 1 - b


def cfg(fid: str, width: int, block_size=(1, 16), skip_first_dim: bool = True) -> dict:
    """The q_config entry of format `fid` at `width` bits."""
    ew, b = FORMATS[fid]
    return dict(name="block_fp", width=width, exponent_width=ew, exponent_bias=b, block_size=list(block_size),
                skip_first_dim=skip_first_dim)


# exponents k of block maxima in (2^(k-1), 2^k] that a dtype holds as normal numbers with room for smaller elements
_K_RANGE = {torch.float32: (-24, 120), torch.bfloat16: (-24, 120), torch.float16: (-11, 15)}
# (fp32 / bf16 from -24: a block wholly below 1e-8 = 2^-26.6 is the pass-through, not the quantizer; up to 2^120 so that a sum of a few
# such values stays finite.  fp16: 2^-11 leaves three binades of normal numbers below the maximum; 2^15 < 65504.)


def classes_for(fid: str, dtype):
    """The k ranges [lo, hi] of the three classes (below emin, inside, above emax) for this dtype; None where it cannot reach one."""
    emin, emax = e_range(fid)
    klo, khi = _K_RANGE[dtype]
    cut = lambda a, b: (max(a, klo), min(b, khi)) if max(a, klo) <= min(b, khi) else None
    return cut(emin - 4, emin - 1), cut(emin, emax), cut(emax + 1, emax + 4)


def class_ks(fid: str, dtype, mid_span: int = 12, far: bool = True):
    """The exponents k each reachable class draws from, as lists (below emin, inside, above emax; an unreachable class is left out).
    A middle wider than `mid_span` stays near the reachable clamp(s), where the interest is; with no reachable clamp it takes the
    format's largest exponents (e8b120: exponent bytes beyond 200) if `far`, else - and for the control - the exponents around 0."""
    low, mid, high = classes_for(fid, dtype)
    out = []
    for i, r in enumerate((low, mid, high)):
        if r is None:
            continue
        ks = list(range(r[0], r[1] + 1))
        if i == 1 and len(ks) > mid_span:
            h = mid_span // 2
            if low is not None and high is not None:
                ks = ks[:h] + ks[-h:]
            elif low is not None:
                ks = ks[:mid_span]
            elif high is not None or (far and FORMATS[fid][1] is not None):
                ks = ks[-mid_span:]
            else:
                ks = list(range(-h, h + 1))
        out.append(ks)
    return out


def _ulp_step(t: torch.Tensor, n: int) -> torch.Tensor:
    """t (positive, a 16- or 32-bit float dtype) moved by n ulps of its own dtype."""
    it = torch.int32 if t.dtype == torch.float32 else torch.int16
    return (t.contiguous().view(it) + n).view(t.dtype)


def ladder(fid: str, dtype, rows: int, cols: int, block: int = 16, seed: int = 0, mid_span: int = 12, far: bool = True) -> torch.Tensor:
    """[rows, cols] tensor of `dtype` on the CPU; blocks of `block` elements along a row (<= 0: the whole row)."""
    g = torch.Generator().manual_seed(1000 * seed + 17)
    L = cols if block <= 0 or block > cols else block
    nb = -(-cols // L)
    ranges = [torch.tensor(ks, dtype=torch.int64) for ks in class_ks(fid, dtype, mid_span, far)]
    n = rows * nb
    cls = torch.arange(n) % len(ranges)
    cls = cls[torch.randperm(n, generator=g)]
    k = torch.empty(n, dtype=torch.int64)
    for c, ks in enumerate(ranges):
        sel = cls == c
        k[sel] = ks[torch.randint(0, len(ks), (int(sel.sum()),), generator=g)]
    x = torch.zeros(rows, nb * L, dtype=torch.float64)
    u = (torch.rand(n, L, generator=g, dtype=torch.float64) * 2 - 1)           # the body of a block: (-1, 1) of its scale
    top = 0.5 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)          # its maximum: (0.5, 1] -> ceil(log2) = k
    top[::5] = 1.0                                                             # every fifth block: exactly the power of two
    pos = torch.randint(0, L, (n,), generator=g)
    u = u * 0.49
    u[torch.arange(n), pos] = top * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    x = (u * torch.pow(2.0, k.double())[:, None]).reshape(rows, nb * L)[:, :cols].contiguous()
    x = x.to(torch.float32).to(dtype)
    # power-of-two maxima one ulp to either side (of this dtype), where that keeps the block's class
    flat = x.reshape(-1)
    idx = (torch.arange(n) // nb) * cols + (torch.arange(n) % nb) * L + pos
    ok = idx < flat.numel()
    ok &= ((torch.arange(n) % nb) * L + pos) < cols
    for j, step in ((5, 1), (10, -1)):
        sel = torch.zeros(n, dtype=torch.bool)
        sel[j::15] = True
        sel &= ok & (top == 1.0)
        if bool(sel.any()):
            v = flat[idx[sel]]
            flat[idx[sel]] = torch.where(v < 0, -_ulp_step(v.abs(), step), _ulp_step(v.abs(), step))
    x = flat.reshape(rows, cols)
    # scattered zeros, one all-zero block, one tiny element in an ordinary block
    z = torch.rand(rows, cols, generator=g) < 0.03
    z.reshape(-1)[idx[ok]] = False  # (never the block maximum: the classes stay as drawn)
    x = torch.where(z, torch.zeros_like(x), x)
    r0 = rows // 2
    x[r0, : min(L, cols)] = 0
    if dtype != torch.float16 and cols >= 2 * L:
        c0 = L + (int(pos[r0 * nb + 1]) + 1) % L
        x[r0, c0] = 5e-9
    return x


def coverage(x: torch.Tensor, c: dict):
    """Fractions of the non-zero blocks of x whose exponent the format `c` clamps at emin / leaves / clamps at emax, from the
    oracle's decomposed exponents of this very input (unclamped: the same width under an 8-bit exponent field)."""
    wide = dict(c, exponent_width=8, exponent_bias=None)
    kw = lambda d: {k: d[k] for k in ("width", "exponent_width", "exponent_bias", "block_size", "skip_first_dim")}
    xf = x.float()
    blk, _ = O._blocks(xf, list(c["block_size"]), c["skip_first_dim"])
    nz = (blk.abs().amax(dim=-1) != 0).reshape(-1)
    _, _, e_c = O.mxint_quantize(xf, **kw(c), decompose=True)
    _, _, e_u = O.mxint_quantize(xf, **kw(wide), decompose=True)
    e_c, e_u = e_c.reshape(-1)[nz], e_u.reshape(-1)[nz]
    ew = c["exponent_width"]
    b = 2 ** (ew - 1) - 1 if c["exponent_bias"] is None else c["exponent_bias"]
    emin, emax = -b, 2 ** ew - 1 - b
    n = max(int(nz.sum()), 1)
    lo = int(((e_u < emin) & (e_c == emin)).sum()) / n
    hi = int(((e_u > emax) & (e_c == emax)).sum()) / n
    un = int(((e_u >= emin) & (e_u <= emax) & (e_c == e_u)).sum()) / n
    assert abs(lo + hi + un - 1.0) < 1e-9, "the oracle's clamped exponent is not clamp(unclamped, emin, emax)"
    return lo, un, hi


def assert_covered(x: torch.Tensor, fid: str, c: dict, dtype=None, floor: float = 0.15):
    """Every class the dtype can reach for this format holds at least `floor` of the non-zero blocks of x under config `c`."""
    dtype = dtype or x.dtype
    lo, un, hi = coverage(x, c)
    want = classes_for(fid, dtype)
    for name, frac, r in (("clamped at emin", lo, want[0]), ("unclamped", un, want[1]), ("clamped at emax", hi, want[2])):
        if r is not None:
            assert frac >= floor, f"{fid} {dtype}: {name} holds {frac:.2f} of the non-zero blocks (< {floor})"
    return lo, un, hi


def oracle_q(x: torch.Tensor, c: dict, decompose: bool = False):
    kw = {k: c[k] for k in ("width", "exponent_width", "exponent_bias", "block_size", "skip_first_dim")}
    return O.mxint_quantize(x.float(), **kw, decompose=decompose)


# ---- integer-valued operands whose products sum exactly (the exact legs of the Linear, matmul and attention tests) ----------------
def ladder_e(fid: str, dtype, n: int, g, mid_span: int = 12) -> torch.Tensor:
    """n target exponents, one third from each reachable class of the format (class_ks; moderate exponents where no clamp is
    reachable, so that products stay finite), shuffled."""
    ks = class_ks(fid, dtype, mid_span, far=False)
    out = torch.tensor([ks[i % len(ks)][int(torch.randint(0, len(ks[i % len(ks)]), (1,), generator=g))] for i in range(n)])
    return out[torch.randperm(n, generator=g)]


def ints(rows: int, cols: int, mmax: int, block: int, g) -> torch.Tensor:
    """Integers in [-mmax, mmax], every block of `block` columns (<= 0: the row) holding +-mmax somewhere."""
    m = torch.randint(-mmax, mmax + 1, (rows, cols), generator=g).float()
    L = cols if block <= 0 else block
    for b0 in range(0, cols, L):
        w = min(L, cols - b0)
        pos = torch.randint(0, w, (rows,), generator=g) + b0
        m[torch.arange(rows), pos] = mmax * (torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1)
    return m


def lg(mmax: int) -> int:
    """ceil(log2(mmax)): the block exponent of integers up to mmax."""
    return (mmax - 1).bit_length() if mmax > 1 else 0


def grid(x: torch.Tensor) -> torch.Tensor:
    """Per non-zero element of x (fp32), the largest power of two that divides it: 2^(exponent of its lowest set bit), fp64."""
    bits = x[x != 0].contiguous().view(torch.int32).to(torch.int64)
    e = ((bits >> 23) & 0xFF) - 127
    m = (bits & 0x7FFFFF) | 0x800000
    tz = torch.zeros_like(m)
    for sh in range(23, 0, -1):
        tz = torch.where((tz == 0) & ((m & ((1 << sh) - 1)) == 0), torch.full_like(tz, sh), tz)
    return torch.pow(2.0, (e - 23 + tz).double())


def exact_steps(a: torch.Tensor, b: torch.Tensor) -> float:
    """Upper bound, in steps of the finest grid of any operand pair, of every partial sum of a @ b (rows of a x columns of b)."""
    one = torch.tensor(1.0, dtype=torch.float64)
    ga = torch.stack([grid(r).min() if bool((r != 0).any()) else one for r in a])
    gb = torch.stack([grid(c).min() if bool((c != 0).any()) else one for c in b.t()])
    return float(((a.abs().double() @ b.abs().double()) / (ga[:, None] * gb[None, :])).max())


def assert_same_finite(y, ref, dtype, what):
    """y equals ref rounded to `dtype` wherever that is finite (at least a tenth of it), and is finite at exactly those places."""
    want = ref.to(dtype)
    fin = torch.isfinite(want.float())
    # (fp16: rows that clamp at emax in x AND w overflow the output; the comparison runs over everything else)
    assert float(fin.float().mean()) >= 0.1, f"{what}: only {float(fin.float().mean()):.2f} of the expected outputs are finite"
    bad = (y.float() != want.float()) & fin
    rows = bad.any(dim=1).nonzero().flatten().tolist()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(fin.sum())} finite outputs differ, in rows {rows[:12]}"
    assert bool(torch.equal(torch.isfinite(y.float()), fin)), f"{what}: finite / non-finite pattern differs"

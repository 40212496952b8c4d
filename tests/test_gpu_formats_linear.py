"""The Linear forward on every GEMM route with narrow block_fp formats (tests/_formats.py) in x, w, A_out, B_out and the bias: two
exact legs per route with no tolerance, and everything together at the project's bars.

Routes: the one-launch decode kernel (M = 3; with LQER_TUNE_DECODE_NO_POLL), the small-M kernel (M = 40), 64- and 128-row tiles
(M = 100 / 130; B_out in the prologue and - K = 1024 - under the main loop; rank 32 direct, rank 48 staged), the 256-row kernel (the
smallest M, N at K = 64 for which lqer_gemm_route says so), the int8 route (per-token x, weight blocks of 128 and of the row, 128-
and 256-row tiles) and both forms of the activation side (LQER_TUNE_ACT16_* / ACT8_*).  Every case asserts the route, the tile rows
and lqer_decode_partials it meant to reach.  K = 320 (five k-steps: past the ring fill), N = 272 (two column tiles, ragged).
The two decode cases and `smallm` assert the same three answers (ROUTE_SMALLM, no tile rows, one partial): that the one-launch kernel
runs at M = 3 is inferred from M <= 8 and a shape inside its limits, not observed - lqer_linear_forward falls back to the two-launch
small-M route without a word where the one-launch dispatch declines (as in tests/test_gpu_decode1.py).

A_out and B_out keep width 8 and vary the exponent field only: their ties under the summation order of x A are a known, separately
bounded effect (tests/_envelope.py), and narrower widths there would need a bar of their own.

(i) Main product alone: A = B = 0 (the side path adds an exact 0; the decode routes need a rank).  x = integer mantissas up to the
width's largest, times 2^a(m) per token row; W = integers up to its width's largest times 2^b(n) per output row (block-128 weights:
b also moves by up to 2 from group to group); every block holds the largest mantissa, so the unclamped block exponent is known, and
a, b walk the format's ladder: below emin, inside, above emax.  Every product and partial sum is an integer multiple of one grid
step per (m, n), below 2^24 steps (asserted on the CPU): the output must be oracle.lqer_linear_forward rounded to the module's dtype,
in fp32, fp16 and bf16, wherever that is finite.
(ii) Side path alone: W = 0, x under the control format, A integer-valued in [-3, 3] times one power of two, B integer-valued in
[-3, 3] times one power of two per block of 16 columns: x A and xAq B are exact - every output element sums on one grid -, so A_out
and B_out see the same numbers in any summation order and y = Q_Bout(Q_Aout(xq A) B) must be the oracle's.  The rows' scales walk
A_out's ladder; the powers of two of B's column blocks are picked so that the block exponents of xAq B walk B_out's, whatever A_out's
clamped range is.  Asserted on the CPU first: every class that A_out's and B_out's formats can reach in the dtype holds 15 % of the
non-zero blocks of x A and of xAq B; both sums stay below 2^24 grid steps.  (The int8 route quantizes one block per token row: the
one exponent B_out sees per row follows A_out's clamped range, so its cases pair formats where that range is the wider one.)
(iii) Everything together: rows of x and of W uniform on the ladders of their formats (fp16: W at the one exponent that keeps every
output normal and finite), a bias on the ladder of a narrow format at x's width - OPT-style blocks of 16, or one block - on the left
half of the columns, and the side path: in fp32 at about 1e-3 of the output, in fp16 / bf16 scaled on the oracle until it is four
times the bar of the row in a third of the rows (see the test; a narrow B_out caps it at 2^emax).  Against the oracle at the project's
bars (tools/fuzz_parity.py): relative L2 1e-3 fp16, 6e-3 bf16, 3e-5 fp32, over the tensor, per token row, and per token row over the
columns without bias; every row is asserted.  The oracle's own rounding to the dtype (kept in fp32 against rounded) takes at most
2.6e-4 (fp16) / 2.6e-3 (bf16) of a row - asserted below the bar in every case, so the bars stand as they are.  Measured worst row:
2.6e-4 fp16, 2.6e-3 bf16, 1.9e-6 fp32 (without bias 2.7e-4, 3.1e-3, 1.6e-6); over the tensor 2.2e-4, 1.8e-3, 1.9e-7.  fp32 rows of
x A with an element within D ulps of an A_out tie (found on the CPU, at most 2.3 % of the rows) may come out one step of xAq apart
under another summation order: the worst measured 3.8e-5 of the row, 9.8e-5 of its half without bias, and they are asserted at
TIE_BAR / TIE_BAR_RIGHT, 4 x those figures.

Equality is torch.equal on the values (a -0 against a +0 counts as equal).
"""
import ctypes as C
import math

import pytest
import torch

import _formats as F
from _envelope import tie_rows
from oracle import lqer_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NARROW = ("e4", "e2", "e1", "e3b6", "e3bm2")  # both clamps inside every dtype


def _tune(*names):
    from lqer_amd import _lib

    t = 0
    for n in names:
        t |= getattr(_lib, "TUNE_" + n)
    return t


# name -> (kind, M, K, N, rank, tuning names, route, tile rows (None: not asserted), decode_partials)
ROUTES = {
    "decode1": ("b16", 3, 320, 272, 32, (), "SMALLM", 0, 1),
    "decode1-nopoll": ("b16", 3, 320, 272, 32, ("DECODE_NO_POLL",), "SMALLM", 0, 1),
    "smallm": ("b16", 40, 320, 272, 32, (), "SMALLM", 0, 1),
    "tile64": ("b16", 100, 320, 272, 32, ("TILE_ROWS_64",), "TILE128", 64, 0),
    "tile64-prologue-r48": ("b16", 100, 320, 272, 48, ("TILE_ROWS_64", "BOUT_IN_PROLOGUE"), "TILE128", 64, 0),
    "tile128": ("b16", 130, 320, 272, 32, ("TILE_ROWS_128",), "TILE128", 128, 0),
    "tile128-r48": ("b16", 130, 320, 272, 48, ("TILE_ROWS_128",), "TILE128", 128, 0),
    "tile128-prologue": ("b16", 130, 320, 272, 32, ("TILE_ROWS_128", "BOUT_IN_PROLOGUE"), "TILE128", 128, 0),
    "tile128-k1024-defer": ("b16", 130, 1024, 272, 32, ("TILE_ROWS_128",), "TILE128", 128, 0),
    "tile128-k1024-prologue": ("b16", 130, 1024, 272, 32, ("TILE_ROWS_128", "BOUT_IN_PROLOGUE"), "TILE128", 128, 0),
    "tile128-act16-split": ("b16", 130, 320, 272, 32, ("TILE_ROWS_128", "ACT16_SPLIT"), "TILE128", 128, 0),
    "tile128-act16-fused": ("b16", 130, 320, 272, 32, ("TILE_ROWS_128", "ACT16_FUSED"), "TILE128", 128, 0),
    "tile256": ("b16", None, 64, None, 32, (), "TILE256", 256, 0),
    "i8-g128-rows128": ("i8g", 130, 320, 272, 32, ("I8_ROWS_128",), "I8", 128, 0),
    "i8-row-rows256": ("i8r", 300, 320, 272, 32, ("I8_ROWS_256",), "I8", 256, 0),
    "i8-g128-act8-split": ("i8g", 130, 320, 272, 32, ("I8_ROWS_128", "ACT8_SPLIT"), "I8", 128, 0),
    "i8-row-act8-fused": ("i8r", 130, 320, 272, 32, ("I8_ROWS_128", "ACT8_FUSED"), "I8", 128, 0),
}
# (x, w, A_out, B_out) per case: x and w as (format, width), A_out / B_out as formats at width 8
COMBOS = [(("e4", 8), ("e4", 4), "e4", "e3b6"), (("e3b6", 4), ("e3bm2", 3), "e3b6", "e4"), (("e3bm2", 8), ("e2", 4), "e2", "e3bm2"),
          (("e1", 6), ("e5b20", 2), "e3bm2", "e1"), (("e5b20", 3), ("e1", 4), "e1", "e2"), (("e2", 2), ("e8b120", 4), "e5b20", "e4"),
          (("e8b120", 8), ("e3b6", 8), "e8b120", "e2"), (("e8", 8), ("e4", 6), "e8", "e8"), (("e4", 6), ("e8", 5), "e4", "e1")]


# the int8 route's A_out and B_out take one block per token row: the one exponent B_out sees per row follows A_out's clamped range
# (emin - 4 .. emax, 4 below because the ladder goes that far), so B_out's three classes fit only where that is wider than B_out's
ROW_COMBOS = [COMBOS[0], COMBOS[3], COMBOS[5], COMBOS[6], COMBOS[8], (("e3bm2", 8), ("e2", 4), "e5b20", "e3bm2")]


def _combos_for(name, n):
    """Two combos per route, rotating; the one-launch decode and small-M kernels take one weight limb (width <= 4)."""
    kind, M = ROUTES[name][0], ROUTES[name][1]
    pool = [c for c in (COMBOS if kind == "b16" else ROW_COMBOS) if not (M is not None and M <= 64 and c[1][1] > 4)]
    return [pool[(2 * n) % len(pool)], pool[(2 * n + 1) % len(pool)]]


def _cases():
    out = []
    for n, name in enumerate(ROUTES):
        for c in _combos_for(name, n):
            for dt in DTYPES:
                if dt == "f16" and not all(f in F.FP16_IDS for f in (c[0][0], c[1][0], c[2], c[3])):
                    continue  # fp16 holds the ladders of F.FP16_IDS only
                out.append(pytest.param(name, c, dt, id=f"{name}-x{F.pair_id(c[0])}-w{F.pair_id(c[1])}-A{c[2]}-B{c[3]}-{dt}"))
    return out


def _qc(kind, c, b=None):
    """The q_config of a case; b: the bias quantizer's config (default: pass-through)."""
    (fx, wx), (fw, ww), fa, fb = c
    xb = [1, 16] if kind == "b16" else [1, -1]
    wb = {"b16": [1, 16], "i8g": [1, 128], "i8r": [1, -1]}[kind]
    return dict(name="flexible_lqer", is_ptq=True, default=False, x_quantizer=F.cfg(fx, wx, xb, True), w_quantizer=F.cfg(fw, ww, wb, False),
                b_quantizer=b or dict(name="passthrough"), A_out_quantizer=F.cfg(fa, 8, xb, True), B_out_quantizer=F.cfg(fb, 8, xb, True))


def _shape(name, c):
    from lqer_amd import _lib, ops

    kind, M, K, N, r, tune, route, rows, dp = ROUTES[name]
    if M is None:  # the 256-row kernel: the smallest (M, N) at K = 64 the plan sends there
        qc = _qc(kind, c)
        none = _lib.QFmt(_lib.Q_PASSTHROUGH, 0, 0, 8, 127)
        for M, N in sorted(((m, n) for m in (512, 768, 1024, 1536, 2048) for n in (256, 512, 1024, 2048, 4096, 8192)), key=lambda t: t[0] * t[1]):
            d = _lib.LinearDesc(K, N, r, 0, ops.make_qfmt(qc["x_quantizer"], "x"), ops.make_qfmt(qc["w_quantizer"], "w"), none,
                                ops.make_qfmt(qc["A_out_quantizer"], "A_out"), ops.make_qfmt(qc["B_out_quantizer"], "B_out"), 0)
            if _lib.lib().lqer_gemm_route(C.byref(d), M, _lib.F16) == _lib.ROUTE_TILE256:
                break
        else:
            raise AssertionError("no (M, N) takes the 256-row kernel")
    return kind, M, K, N, r, _tune(*tune), route, rows, dp


def _run(name, c, dtype, x, W, A, B, bias=None, bq=None):
    """The module's output for CPU tensors of `dtype`, after asserting the route the case is about (bias, bq: a bias and its quantizer)."""
    import lqer_amd
    from lqer_amd import _lib

    kind, M, K, N, r, tuning, route, rows, dp = _shape(name, c)
    qc = _qc(kind, c, bq)
    mod = lqer_amd.LinearFlexibleLqer(K, N, bias=bias is not None, q_config=qc, l_config={"rank": r})
    mod.load_state_dict(dict({"weight": W.float(), "A": A.float(), "B": B.float()}, **({} if bias is None else {"bias": bias.float()})))
    mod = mod.to(DEV).to(dtype)
    mod.tuning = tuning
    y = mod(x.to(DEV))
    L = _lib.lib()
    dtc = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}[dtype]
    d = mod._desc()
    assert L.lqer_gemm_route(C.byref(d), M, dtc) == getattr(_lib, "ROUTE_" + route), (name, L.lqer_gemm_route(C.byref(d), M, dtc))
    assert L.lqer_gemm_tile_rows(C.byref(d), M, dtc) == rows, (name, L.lqer_gemm_tile_rows(C.byref(d), M, dtc))
    assert L.lqer_decode_partials(C.byref(d), M) == dp, name
    return y.cpu(), qc


@pytest.mark.parametrize("name,c,dt", _cases())
def test_main_product_exact(name, c, dt):
    dtype = DTYPES[dt]
    kind, M, K, N, r, *_ = _shape(name, c)
    (fx, wx), (fw, ww), fa, fb = c
    g = torch.Generator().manual_seed(7)
    xm, wm = 2 ** (wx - 1) - 1, 2 ** (ww - 1) - 1
    ex, ew = F.ladder_e(fx, dtype, M, g), F.ladder_e(fw, dtype, N, g)
    xb, wblk = (16, 16) if kind == "b16" else (-1, 128 if kind == "i8g" else -1)
    x = F.ints(M, K, xm, xb, g) * torch.pow(2.0, (ex - F.lg(xm)).float())[:, None]
    wscale = (ew - F.lg(wm)).float()[:, None].expand(N, K).clone()
    if kind == "i8g" and ww <= 4:  # the exponent moves by up to 2 from one group of 128 to the next (the image of 8-bit codes takes one per row)
        wscale += (torch.arange(K) // 128 % 3).float()[None, :] * (torch.arange(N) % 2).float()[:, None]
    W = F.ints(N, K, wm, wblk, g) * torch.pow(2.0, wscale)
    x[M // 2, :16] = 0
    x[torch.rand(M, K, generator=g) < 0.02] = 0
    x, W = x.to(dtype), W.to(dtype)
    assert bool(torch.isfinite(x.float()).all() and torch.isfinite(W.float()).all())
    A, B = torch.zeros(K, r), torch.zeros(r, N)
    qc = _qc(kind, c)
    if fx in NARROW or dt != "f16":
        F.assert_covered(x, fx, qc["x_quantizer"], dtype)
    F.assert_covered(W, fw, qc["w_quantizer"], dtype)
    out = O.lqer_linear_forward(x.float(), W.float(), None, A, B, qc, intermediates=True)
    steps = F.exact_steps(out["xq"], out["wq"].t())
    assert steps < 2.0 ** 24, f"the main product needs {steps:.3g} grid steps: not exact in fp32"
    y, _ = _run(name, c, dtype, x, W, A, B)
    F.assert_same_finite(y, out["y"], dtype, f"{name} main product")


def _block_e(t, L):
    """ceil(log2) of the largest magnitude of every block of L columns (<= 0: the row) of t [M, N] -> [M, blocks]; -999 for a zero block."""
    M, N = t.shape
    L = N if L <= 0 else L
    nb = -(-N // L)
    a = torch.zeros(M, nb * L)
    a[:, :N] = t.abs()
    amax = a.reshape(M, nb, L).amax(dim=-1)
    return torch.where(amax > 0, O.ceil_log2_f32(torch.where(amax > 0, amax, torch.ones_like(amax))).long(), torch.full_like(amax, -999).long())


def _spread(eu, fid, dtype, ps):
    """One power of two p per column block of B, picked block after block so that the block exponents eu[:, j] + p leave the smallest of
    B_out's reachable classes (F.classes_for) as full as possible.  eu: _block_e of xAq B at p = 0."""
    emin, emax = F.e_range(fid)
    reach = [r is not None for r in F.classes_for(fid, dtype)]
    tot, out = [0, 0, 0], []
    for j in range(eu.shape[1]):
        e = eu[:, j][eu[:, j] > -999]
        best = None
        for p in ps:
            n = [int((e + p < emin).sum()), int(((e + p >= emin) & (e + p <= emax)).sum()), int((e + p > emax).sum())]
            key = sorted(t + k for t, k, ok in zip(tot, n, reach) if ok)
            if best is None or key > best[0]:
                best = (key, p, n)
        tot = [t + k for t, k in zip(tot, best[2])]
        out.append(best[1])
    return torch.tensor(out)


@pytest.mark.parametrize("name,c,dt", _cases())
def test_side_path_exact(name, c, dt):
    dtype = DTYPES[dt]
    kind, M, K, N, r, *_ = _shape(name, c)
    (fx, wx), (fw, ww), fa, fb = c
    g = torch.Generator().manual_seed(11)
    qc = dict(_qc(kind, c), x_quantizer=F.cfg("e8", 8, [1, 16] if kind == "b16" else [1, -1], True))  # x: the control, exact on integers
    c = (("e8", 8), c[1], fa, fb)
    # x A of a row with mantissas up to 127 is about 127 x 2 x sqrt(K) ~ 2^12.x: its block exponent is close to a + 13.  Where the
    # ladder goes below 2^-12 (e5b20), A carries 2^pA so that x itself stays above the pass-through range |x| <= 1e-8
    # (one block per token row - the int8 route: the rows of a narrow middle stay at its two ends, so that enough of them land in a
    # B_out range of two exponents)
    ea = F.ladder_e(fa, dtype, M, g, mid_span=4 if kind != "b16" and any(r is not None for r in F.classes_for(fa, dtype)[::2]) else 12)
    pA = min(0, int(ea.min()) + 12)
    A = torch.randint(-3, 4, (K, r), generator=g).float() * 2.0 ** pA
    B0 = torch.randint(-3, 4, (r, N), generator=g).float()
    lg_xa = math.ceil(math.log2(127 * 2 * math.sqrt(K)))
    x = F.ints(M, K, 127, 16 if kind == "b16" else -1, g) * torch.pow(2.0, (ea - lg_xa - pA).float())[:, None]
    x = x.to(dtype)
    assert torch.equal(x.float().to(dtype).float(), x.float()) and bool(torch.isfinite(x.float()).all())
    assert not bool(((x.float() != 0) & (x.float().abs() <= 1e-8)).any())
    qs = O.resolve_linear_quantizers(qc)
    xq = O.get_quantizer(qs["x"])(x.float())
    assert torch.equal(xq, x.float()), "x is not a fixed point of the control quantizer"
    xA = xq @ A
    # (an element of x A inside the reference's pass-through range |v| <= 1e-8 - e5b20's lowest blocks hold some - is 0 in the
    # image of xAq, as in every packed image: the declared difference)
    xAq = torch.where(xA.abs() <= 1e-8, torch.zeros_like(xA), O.get_quantizer(qs["A_out"])(xA))
    F.assert_covered(xA, fa, qc["A_out_quantizer"], dtype)
    # B: every block of 16 columns (the int8 route: the whole matrix) carries its own power of two, so that each output element still
    # sums on one grid and B_out's block exponents walk its ladder whatever A_out's clamped range is
    Lb = 16 if kind == "b16" else -1
    ps = range(-12, 13) if dtype == torch.float16 else range(-48, 49)
    p = _spread(_block_e(xAq @ B0, Lb), fb, dtype, ps)
    B = B0 * torch.pow(2.0, p.float()).repeat_interleave(16 if Lb > 0 else N)[None, :N]
    assert torch.equal(B.to(dtype).float(), B)
    xAB = xAq @ B
    F.assert_covered(xAB, fb, qc["B_out_quantizer"], dtype)
    ref = O.get_quantizer(qs["B_out"])(xAB)
    for what, a, b in (("x A", xq, A), ("xAq B", xAq, B)):
        steps = F.exact_steps(a, b)
        assert steps < 2.0 ** 24, f"{what} needs {steps:.3g} grid steps: not exact in fp32"
    y, _ = _run(name, c, dtype, x, torch.zeros(N, K), A, B)
    F.assert_same_finite(y, ref, dtype, f"{name} side path")


# ---- (iii) everything together ------------------------------------------------------------------------------------------------------
BARS = {"f16": 1e-3, "bf16": 6e-3, "f32": 3e-5}  # relative L2 against the oracle: the project's forward bars
SHARE = {"f16": 4e-3, "bf16": 2.4e-2}  # the part of an output row at which the side product counts as seen: 4 x the bar
TIE_BAR, TIE_BAR_RIGHT = 4 * 3.8e-5, 4 * 9.8e-5  # fp32 rows on a tie of A_out: 4 x the measured distance (see the test)


def _cases3():
    out = []
    for n, name in enumerate(ROUTES):
        for i, c in enumerate(_combos_for(name, n)):
            for dt in DTYPES:
                if dt == "f16" and not all(f in F.FP16_IDS for f in (c[0][0], c[1][0], c[2], c[3])):
                    continue
                blocks = "opt" if i == 0 else "whole"  # OPT-style bias blocks of 16 / one block over the bias
                out.append(pytest.param(name, c, dt, blocks, id=f"{name}-x{F.pair_id(c[0])}-w{F.pair_id(c[1])}-A{c[2]}-B{c[3]}-b{blocks}-{dt}"))
    return out


def _rand_rows(e, cols, block, g):
    """[len(e), cols]: row i uniform in (-0.49, 0.49) 2^e[i], every block of `block` columns (<= 0: the row) holding one +-[0.51, 1] 2^e[i]
    (from 0.51: rounding to bf16 must not reach 0.5, the next exponent down)."""
    rows = len(e)
    t = (torch.rand(rows, cols, generator=g) * 2 - 1) * 0.49
    L = cols if block <= 0 else block
    for b0 in range(0, cols, L):
        pos = torch.randint(0, min(L, cols - b0), (rows,), generator=g) + b0
        t[torch.arange(rows), pos] = (0.51 + 0.49 * torch.rand(rows, generator=g)) * (torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1)
    return t * torch.pow(2.0, e.float())[:, None]


def _oracle_flushed(x, W, b, A, B, qc, parts=False):
    """oracle.lqer_linear_forward with the declared difference of every packed image: an element |v| <= 1e-8 of x, of W and of x A,
    which the reference leaves unquantized, is 0.  The ladders of e5b20 go down to 2^-24, where a third of a row lies in that range -
    under the reference's rule such a row would consist of what the quantizer passed through.  Without such elements this is
    lqer_linear_forward itself, bit for bit (asserted).  parts: return (x W + b, xAq, the B_out quantizer) instead, for trying several B."""
    qs = O.resolve_linear_quantizers(qc)
    flush = lambda v, q: torch.where(v.abs() <= 1e-8, torch.zeros_like(q), q)
    tiny = lambda v: bool(((v != 0) & (v.abs() <= 1e-8)).any())
    xq, wq = flush(x, O.get_quantizer(qs["x"])(x)), flush(W, O.get_quantizer(qs["w"])(W))
    xA = xq @ A
    xAq = flush(xA, O.get_quantizer(qs["A_out"])(xA))
    if parts:
        return torch.nn.functional.linear(xq, wq, O.get_quantizer(qs["b"])(b)), xAq, O.get_quantizer(qs["B_out"])
    y = torch.nn.functional.linear(xq, wq, O.get_quantizer(qs["b"])(b)) + O.get_quantizer(qs["B_out"])(xAq @ B)
    if not (tiny(x) or tiny(W) or tiny(xA)):
        assert torch.equal(y, O.lqer_linear_forward(x, W, b, A, B, qc))
    return y


def _row_rel(y, ref):
    """Relative L2 per row, over the rows where the reference is not 0."""
    den = ref.double().norm(dim=1)
    return ((y.double() - ref.double()).norm(dim=1) / den.clamp_min(1e-300))[den > 0]


@pytest.mark.parametrize("name,c,dt,blocks", _cases3())
def test_everything_together(name, c, dt, blocks):
    """Random operands on the ladders, a bias (OPT-style blocks of 16, or one block) and the side path at once, against the oracle at
    the project's bars - over the tensor, per token row, and per token row over the columns that carry no bias."""
    dtype = DTYPES[dt]
    kind, M, K, N, r, *_ = _shape(name, c)
    (fx, wx), (fw, ww), fa, fb = c
    g = torch.Generator().manual_seed(13)
    ex, ew = F.ladder_e(fx, dtype, M, g), F.ladder_e(fw, dtype, N, g)
    xtop, wtop = F.e_range(fx)[1], F.e_range(fw)[1]
    if dtype == torch.float16:
        # fp16 outputs stay finite and normal: an element of x W is about 1.5 x 2^(ex + ew) and at most some 8 x 2^(ex + ew) (320 products
        # of two uniform numbers), ex and ew after the upper clamps.  x keeps its whole ladder; every row of W sits at the one exponent
        # that puts the largest rows near 2^11 .. 2^14 - the smallest, 2^-11 in x, then still lie near 2^-8
        ew = torch.full_like(ew, 11 - math.ceil(0.5 * math.log2(K / 320)) - min(int(ex.max()), xtop))  # (K = 320: 11; the sums grow as sqrt(K))
    xb, wblk = (16, 16) if kind == "b16" else (-1, 128 if kind == "i8g" else -1)
    x = _rand_rows(ex, K, xb, g).to(dtype)
    W = _rand_rows(ew, K, wblk, g).to(dtype)
    x[M // 2, :16] = 0
    bqc = F.cfg(fa, wx, [1, 16] if blocks == "opt" else [-1], False)
    bias = F.ladder(fa, dtype, 1, N, 16, seed=3, far=False)[0]
    bias[N // 2:] = 0  # (the right half of the columns: x W and the side path alone)
    # the side path.  fp32: B at 2^-5, about 1e-3 of the output.  fp16 / bf16: B times the smallest power of two at which the side
    # product is at least SHARE - four times the bar - of the output row in a third of the rows (found on the oracle; a narrow B_out
    # caps the side product at 2^emax whatever the row's scale, so the largest rows never see it - where a third is out of reach the
    # best power of two is taken, and a tenth of the rows asserted).  An output without the side product then misses the bar four times
    # over in those rows, while one step of xAq under another summation order of x A (tests/_envelope.py: 2^-7 of the block maximum,
    # some 3.5e-3 of the row of xAq, 2^4 times that 4 below emin) mostly stays under it next to the rounding of the output
    A = (torch.randn(K, r, generator=g) * 0.3 / math.sqrt(K)).to(dtype)
    B0 = torch.randn(r, N, generator=g) * 0.3 * torch.pow(2.0, torch.minimum(ew, torch.tensor(wtop)).float())[None, :]
    qc = _qc(kind, c, bqc)
    main, xAq, qb = _oracle_flushed(x.float(), W.float(), bias.float(), A.float(), B0, qc, parts=True)

    def seen(p):
        """Fraction of the rows in which the side product under B0 2^p is SHARE of the output row or more."""
        side = qb(xAq @ (B0 * 2.0 ** p).to(dtype).float())
        h = slice(N // 2, N)  # (the columns without bias, whose per-row figure is asserted too: a bias at 2^emax hides any side product)
        return float((side[:, h].norm(dim=1) >= SHARE.get(dt, 0.0) * (main + side)[:, h].norm(dim=1)).float().mean())

    if dt == "f32":
        pB = -5
    else:
        fr = {p: seen(p) for p in range(-12, 9)}
        pB = min((p for p in fr if fr[p] >= 1 / 3), default=max(fr, key=fr.get))
        # (where not even a side product at B_out's largest value in every column would be SHARE of a tenth of the rows, the formats
        # of the case cannot show it at this bar - a B_out of [0, 1] beside weights up to 2^11 -, and leg (ii) is what covers it)
        h = slice(N // 2, N)
        cap = float((math.sqrt(N - N // 2) * 2.0 ** F.e_range(fb)[1] >= SHARE[dt] * main[:, h].norm(dim=1)).float().mean())
        assert fr[pB] >= 0.1 or cap < 0.1, f"the side product reaches {SHARE[dt]:.1e} of the output row in {fr[pB]:.2f} of the rows at best ({cap:.2f} within B_out's range)"
    B = (B0 * 2.0 ** pB).to(dtype)
    share = seen(pB)
    assert all(bool(torch.isfinite(t.float()).all()) for t in (x, W, bias, A, B))
    if fx in NARROW or dt != "f16":
        F.assert_covered(x, fx, qc["x_quantizer"], dtype)
    if dt != "f16":
        F.assert_covered(W, fw, qc["w_quantizer"], dtype)
    ref = _oracle_flushed(x.float(), W.float(), bias.float(), A.float(), B.float(), qc)
    assert bool(torch.isfinite(ref.to(dtype).float()).all())
    bar = BARS[dt]
    own = float(_row_rel(ref.to(dtype).float(), ref).max())  # the oracle against itself: rounded to the dtype against kept in fp32
    assert own <= bar, f"the oracle's own rounding to {dt} takes {own:.2e} of a row: the bar {bar:.0e} is not admissible there"
    # fp32: rows of x A with an element within D ulps of a rounding tie of A_out (tests/_envelope.py: D = max(16, sqrt K)).  Another
    # summation order may give another xAq there, one step apart, and B_out then re-quantizes another row: in the one such row
    # measured, 69 of 8192 outputs lay one step of a B_out clamped 6 below emin apart, 3.8e-5 of the row (9.8e-5 of its half without
    # bias).  Those rows are found on the CPU, are few (asserted) and take TIE_BAR / TIE_BAR_RIGHT, 4 x the measured figures; every
    # other row, and every row in fp16 / bf16, takes the bar itself
    ties = torch.zeros(M, dtype=torch.bool)
    if dt == "f32":
        xq = torch.where(x.float().abs() <= 1e-8, torch.zeros_like(x.float()), O.get_quantizer(O.resolve_linear_quantizers(qc)["x"])(x.float()))
        ties = torch.from_numpy(tie_rows(xq.double().numpy() @ A.double().numpy(), 16 if kind == "b16" else r, 7, max(16.0, math.sqrt(K)), *F.e_range(fa)))
        assert float(ties.float().mean()) <= 0.05, f"{int(ties.sum())} of {M} rows of x A sit on a tie of A_out"
    y, _ = _run(name, c, dtype, x, W, A, B, bias, bqc)
    y = y.float()
    whole = float((y - ref).norm() / ref.norm())
    worst = lambda yy, rr, sel: float(_row_rel(yy[sel], rr[sel]).max()) if bool(sel.any()) else 0.0
    rows, right = worst(y, ref, ~ties), worst(y[:, N // 2:], ref[:, N // 2:], ~ties)
    trows, tright = worst(y, ref, ties), worst(y[:, N // 2:], ref[:, N // 2:], ties)
    print(f"together {name} {dt}: rel-L2 {whole:.2e}, worst row {rows:.2e}, worst row without bias {right:.2e} (oracle's own rounding {own:.2e}, "
          f"bar {bar:.0e}, side product seen in {share:.2f} of the rows; {int(ties.sum())} of {M} rows on a tie of A_out: {trows:.2e}, without bias {tright:.2e})")
    assert bool(torch.isfinite(y).all())
    assert whole <= bar and rows <= bar and right <= bar
    assert trows <= TIE_BAR and tright <= TIE_BAR_RIGHT

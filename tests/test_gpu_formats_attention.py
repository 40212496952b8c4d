"""Fused quantized attention (lqer_attention_q: prefill; lqer_attention_q_decode: up to 8 query rows, split over the keys) and the
packed KV caches (dense and paged) with four DIFFERENT block_fp formats for Q, K^T, P and V: narrow exponent fields whose clamps are
met at both ends, widths 2 .. 8 (tests/_formats.py).  Every other attention / KV test runs the one all-width-8, 8-bit-exponent config
tests/golden/matmul_config.json.

The comparator is tests/_attention.py's (the one of tests/test_gpu_attention_fused.py), given the two configs.  The bar on O is the project's forward bar, relative
L2 <= 1e-3.  It is admissible only where the comparator's own spread - the same construction with fp64 products and an fp64 softmax
(comparator(..., acc=torch.float64)) - is at most 1e-4, a margin of 10: every parity case computes that spread on the CPU, prints it
and asserts it BEFORE its first GPU call; seeds and q / k scales were chosen on the CPU alone so that it holds (SEEDS; bf16 keeps q / k
at scale 1, see _parity_cases).  Worst own spread per quadruple over its parity cases, measured on the CPU at the committed seeds:

    quadruple      Q        K^T        P        V         fp16   bf16   fp32
    narrowP-e3b6   e8/8     e4/8       e3b6/8   e5b20/8   0      0      1.5e-8
    narrowP-e1     e4/8     e8/8       e1/8     e4/6      0      0      2.0e-8
    kv-e3bm2-e2    e8/8     e3bm2/8    e4/8     e2/8      0      0      0
    all-w4         e8/4     e4/4       e3b6/4   e5b20/4   0      0      2.1e-8
    mixed-8463     e4/8     e5b20/4    e8/6     e3b6/3    0      0      4.1e-8
    kv-e2-e3bm2    e5b20/6  e2/8       e3b6/8   e3bm2/6   0      0      2.8e-8
    wide-bias      e3b6/8   e8b120/6   e2/8     e8/3      0      0      0
    narrow-all     e2/6     e1/8       e5b20/8  e1/4      0      0      7.1e-5
(0: the two evaluations round to the same 16-bit outputs.  All-width-2 is left out: its spread was 1.6e-4 in bf16.)

The exact leg: q and k integer-valued in [-15, 15] times one power of two per case - 2^pk puts the block exponents of K^T at
emax - 2 .. emax + 2 wherever the K format's emax is reachable, so part of its blocks clamp there and saturate -, quantization is
deterministic, and every score sum is exact in any order: the test asserts on the CPU that sum |q_i k_i| over the operands' common
grid stays below 2^24.  row_stats[..., 0] then equals the comparator's row maximum bit for bit, the row sum to 1e-6 (the width-8
tests' figures).

The KV caches store the outputs of the K^T and V quantizers, so those checks are equalities of bits: stored values against the
oracle (the declared |x| <= 1e-8 flush applied), chunked appends against one append, attention over the cache against the raw
kernels with the same four formats, the paged pool against the dense cache.
"""
import pytest
import torch

import _formats as F
import _attention as A
from oracle import lqer_oracle as O

pytestmark = pytest.mark.gpu

DEV, BAR, SPREAD_MAX = A.DEV, A.BAR, 1e-4
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}

# (Q, K^T, P, V) as (format id, width)
QUADS = {
    "narrowP-e3b6": (("e8", 8), ("e4", 8), ("e3b6", 8), ("e5b20", 8)),
    "narrowP-e1": (("e4", 8), ("e8", 8), ("e1", 8), ("e4", 6)),
    "kv-e3bm2-e2": (("e8", 8), ("e3bm2", 8), ("e4", 8), ("e2", 8)),
    "all-w4": (("e8", 4), ("e4", 4), ("e3b6", 4), ("e5b20", 4)),
    "mixed-8463": (("e4", 8), ("e5b20", 4), ("e8", 6), ("e3b6", 3)),
    "kv-e2-e3bm2": (("e5b20", 6), ("e2", 8), ("e3b6", 8), ("e3bm2", 6)),
    "wide-bias": (("e3b6", 8), ("e8b120", 6), ("e2", 8), ("e8", 3)),
    "narrow-all": (("e2", 6), ("e1", 8), ("e5b20", 8), ("e1", 4)),
}


def cfgs(quad):
    """The two matmul configs of a quadruple: blocks of 16 along the last dim of each operand."""
    c = [F.cfg(fid, w, [1, 16], True) for fid, w in QUADS[quad]]
    return (dict(name="flexible", default=c[0], x_quantizer=c[0], w_quantizer=c[1]),
            dict(name="flexible", default=c[2], x_quantizer=c[2], w_quantizer=c[3]))


def _fused(q, k, v, cfg0, cfg1, scaling, mask=None, causal=False, kernel=None):
    from lqer_amd import attention_flexible

    assert attention_flexible.route(q, k, v, cfg0, cfg1, mask, causal) == "fused"
    return attention_flexible(q, k, v, cfg0, cfg1, scaling, attention_mask=mask, causal=causal, return_stats=True, kernel=kernel)


def _kernel_for(s):
    return "decode" if s <= 8 else "prefill"


# ---- 1. the exact leg ---------------------------------------------------------------------------------------------------------
def _exact_scales(quad, d):
    """(pq, pk): q = integers 2^pq, k = integers 2^pk.  pk = emax_k - 2 where fp16 can hold 15 x 2^pk (block exponents pk .. pk + 4
    straddle emax: the larger blocks clamp and saturate), else 0; pq keeps Q inside its format and the scores small."""
    (fq, _), (fk, _), _, _ = QUADS[quad]
    emin_q, emax_q = F.e_range(fq)
    _, emax_k = F.e_range(fk)
    pk = emax_k - 2 if emax_k <= 11 else 0
    pq = max(min(emax_q - 4, -pk - 2), emin_q - 2)
    return pq, pk


EXACT_SHAPES = [(2, 4, 2, 70, 150, 48), (1, 4, 2, 33, 77, 128), (2, 2, 2, 5, 37, 16), (2, 8, 2, 8, 300, 48)]  # b, h, hk, s, t, d


def _exact_cases():
    out = []
    for quad in QUADS:
        for i, shape in enumerate(EXACT_SHAPES):
            pq, pk = _exact_scales(quad, shape[5])
            for dt in DTYPES:
                if dt == "f16" and 225.0 * shape[5] * 2.0 ** (pq + pk) >= 60000:
                    continue  # the unscaled scores, which every route rounds to the dtype, would leave fp16
                mode = ("causal", "mask", "none")[(i + len(out)) % 3]
                out.append(pytest.param(quad, shape, dt, mode, id=f"{quad}-{'x'.join(map(str, shape))}-{dt}-{mode}"))
    return out


@pytest.mark.parametrize("quad,shape,dt,mode", _exact_cases())
def test_exact_scores(quad, shape, dt, mode):
    b, h, hk, s, t, d = shape
    dtype = DTYPES[dt]
    cfg0, cfg1 = cfgs(quad)
    pq, pk = _exact_scales(quad, d)
    g = torch.Generator().manual_seed(5)
    q = (torch.randint(-15, 16, (b, h, s, d), generator=g).float() * 2.0 ** pq).to(dtype)
    # (k: the bound of every block of 16 keys at one d is 1, 3, 7 or 15, so that the blocks' exponents spread over pk + 1 .. pk + 4)
    bound = 2 ** torch.randint(1, 5, (b, hk, (t + 15) // 16, 1, d), generator=g) - 1
    bound = bound.expand(b, hk, (t + 15) // 16, 16, d).reshape(b, hk, -1, d)[:, :, :t]
    k = torch.round((torch.rand(b, hk, t, d, generator=g) * 2 - 1) * bound)
    k = (k * 2.0 ** pk).to(dtype)
    v = A._randn((b, hk, t, d), dtype, 4)
    assert torch.equal(q.float(), q.float().to(dtype).float()) and bool(torch.isfinite(k.float()).all())
    # conditions on the oracle, before any GPU call: part of the K^T blocks clamp at emax; the score sums are exact in any order
    kt = k.float().reshape(b * hk, t, d).transpose(1, 2).contiguous()
    qq = O.get_quantizer(cfg0["x_quantizer"])(q.float().reshape(b * h, s, d))
    kq = O.get_quantizer(cfg0["w_quantizer"])(kt)
    if F.e_range(QUADS[quad][1][0])[1] <= 11:
        lo, un, hi = F.coverage(kt, cfg0["w_quantizer"])
        assert hi >= 0.15 and un >= 0.15, (lo, un, hi)
    gq, gk = float(F.grid(qq).min()), float(F.grid(kq).min())
    rep = kq.reshape(b, hk, 1, d, t).expand(b, hk, h // hk, d, t).reshape(b * h, d, t)
    bits = float((qq.abs().double() @ rep.abs().double()).max()) / (gq * gk)
    assert bits < 2.0 ** 24, f"score sums need {bits:.3g} grid steps: not exact in fp32"
    scaling = d ** -0.5 * 2.0 ** -(pq + pk + 3)
    mask = A._mask(mode, b, s, t, dtype)
    ref, S2, _ = A.comparator(q, k, v, scaling, mask, cfg0, cfg1)
    want_max = S2.float().amax(dim=-1)
    assert bool(torch.isfinite(want_max).all()) and float(S2.float().abs().max()) > 0
    gm = None if mask is None or mode == "causal" else mask.to(DEV)
    got, stats = _fused(q.to(DEV), k.to(DEV), v.to(DEV), cfg0, cfg1, scaling, gm, mode == "causal", _kernel_for(s))
    stats = stats.cpu()
    assert torch.equal(stats[..., 0], want_max), f"row max differs in {(stats[..., 0] != want_max).sum().item()} of {want_max.numel()} rows"
    want_sum = torch.exp((S2.float() - want_max[..., None]).double()).sum(-1)
    rel = ((stats[..., 1].double() - want_sum).abs() / want_sum).max().item()
    print(f"exact leg {quad} {shape} {dt} {mode}: row-sum rel {rel:.2e}, O rel-L2 {A._rel(got.cpu().float(), ref.float()):.2e}")
    assert rel <= 1e-6


# ---- 2. parity against the comparator, fused against unfused ---------------------------------------------------------------------
PREFILL = [(2, 4, 2, 70, 150, 48, 1.0, "causal"), (1, 4, 4, 100, 203, 64, 3.0, "causal"), (2, 2, 1, 40, 90, 16, 1.0, "mask"), (1, 4, 2, 33, 77, 128, 1.0, "none")]
DECODE = [(2, 4, 2, 5, 37, 48, 1.0, "mask"), (2, 8, 2, 8, 300, 16, 3.0, "causal"), (1, 4, 4, 1, 300, 128, 1.0, "none"), (2, 4, 2, 3, 37, 128, 1.0, "causal")]
# seeds chosen on the CPU so that the comparator's own spread stays at or below 1e-4 (default 10)
SEEDS = {
    ("kv-e2-e3bm2", (1, 4, 4, 100, 203, 64, 3.0, "causal"), "f32"): 40,  # seed 10: own spread 2.6e-4; seed 40: 1.9e-8
    ("narrow-all", (2, 4, 2, 70, 150, 48, 1.0, "causal"), "f16"): 40,    # seed 10: 1.35e-4; seed 40: 0
}


def _parity_cases():
    out = []
    for n, quad in enumerate(QUADS):
        for case in (PREFILL[n % 4], PREFILL[(n + 1) % 4], DECODE[n % 4], DECODE[(n + 2) % 4]):
            for dt in DTYPES:
                # bf16 keeps q / k at scale 1: at scale 3 the softmax is sharp enough that one rounding of S to bf16's 8 bits moves a whole
                # row, and the comparator's own spread was 2.8e-4 .. 4.2e-4 at every one of 50 seeds for narrowP-e1 and all-w4
                c = case[:6] + (1.0,) + case[7:] if dt == "bf16" else case
                out.append(pytest.param(quad, c, dt, id=f"{quad}-{'x'.join(map(str, c))}-{dt}"))
    return out


@pytest.mark.parametrize("quad,case,dt", _parity_cases())
def test_parity_vs_comparator_and_unfused(quad, case, dt):
    from lqer_amd import functional

    b, h, hk, s, t, d, sc, mode = case
    dtype = DTYPES[dt]
    cfg0, cfg1 = cfgs(quad)
    seed = SEEDS.get((quad, case, dt), 10)
    q, k, v = A._randn((b, h, s, d), dtype, seed, sc), A._randn((b, hk, t, d), dtype, seed + 1, sc), A._randn((b, hk, t, d), dtype, seed + 2)
    scaling = d ** -0.5
    mask = A._mask(mode, b, s, t, dtype)
    ref, _, _ = A.comparator(q, k, v, scaling, mask, cfg0, cfg1)
    ref64, _, _ = A.comparator(q, k, v, scaling, mask, cfg0, cfg1, acc=torch.float64)
    spread = A._rel(ref, ref64)
    print(f"own spread {quad} {case} {dt}: {spread:.2e}")
    assert spread <= SPREAD_MAX, f"the comparator's own spread {spread:.2e} leaves no margin of 10 under the bar: another draw"
    gq, gk, gv = q.to(DEV), k.to(DEV), v.to(DEV)
    gm = None if mask is None else mask.to(DEV)
    got, _ = _fused(gq, gk, gv, cfg0, cfg1, scaling, None if mode == "causal" else gm, mode == "causal", _kernel_for(s))
    err = A._rel(got.cpu(), ref)
    unf, _ = functional.unfused_attention(gq, gk, gv, cfg0, cfg1, scaling, gm)
    err_u = A._rel(got, unf)
    print(f"parity {quad} {case} {dt}: O rel-L2 vs comparator {err:.3e}, vs the unfused route {err_u:.3e}")
    assert bool(torch.isfinite(got).all())
    assert err <= BAR
    assert err_u <= BAR


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("quad", ["narrowP-e1", "mixed-8463"])
@pytest.mark.parametrize("s,t,d", [(70, 150, 48), (5, 300, 64)])
def test_causal_equals_mask_tensor(quad, dt, s, t, d):
    dtype = DTYPES[dt]
    cfg0, cfg1 = cfgs(quad)
    q, k, v = (x.to(DEV) for x in (A._randn((2, 4, s, d), dtype, 30, 2.0), A._randn((2, 2, t, d), dtype, 31, 2.0), A._randn((2, 2, t, d), dtype, 32)))
    a, sa = _fused(q, k, v, cfg0, cfg1, d ** -0.5, causal=True, kernel=_kernel_for(s))
    m, sm = _fused(q, k, v, cfg0, cfg1, d ** -0.5, mask=A._causal_mask(s, t, dtype).to(DEV), kernel=_kernel_for(s))
    assert torch.equal(a, m) and torch.equal(sa, sm)


# ---- 3. the packed KV cache, dense and paged ------------------------------------------------------------------------------------------
KV_PAIRS = [("e4", 8, "e5b20", 8), ("e3bm2", 8, "e2", 8), ("e4", 4, "e5b20", 4), ("e5b20", 4, "e3b6", 3), ("e2", 8, "e3bm2", 6), ("e8b120", 6, "e8", 3),
            ("e1", 8, "e1", 4), ("e8", 2, "e4", 2), ("e3b6", 6, "e4", 6)]


def _kv_cfgs(fk, wk, fv, wv):
    x = F.cfg("e8", 8, [1, 16], True)
    return (dict(name="flexible", default=x, x_quantizer=x, w_quantizer=F.cfg(fk, wk, [1, 16], True)),
            dict(name="flexible", default=x, x_quantizer=x, w_quantizer=F.cfg(fv, wv, [1, 16], True)))


def _kv_ladder(fk, fv, dtype, b, hk, t, d, seed):
    """K whose transposed rows [d, t] and V whose rows [t, d] are format ladders: the ladder runs along the keys for K^T."""
    kt = F.ladder(fk, dtype, b * hk * d, t, 16, seed=seed)
    v = F.ladder(fv, dtype, b * hk * t, d, 16, seed=seed + 1)
    return kt.reshape(b, hk, d, t).transpose(2, 3).contiguous(), v.reshape(b, hk, t, d).contiguous()


def _kv_oracle(k, v, cfg0, cfg1):
    b, hk, t, d = k.shape
    flush = lambda x, y: torch.where(x.abs() <= 1e-8, torch.zeros_like(y), y)
    kt = k.float().reshape(b * hk, t, d).transpose(1, 2).contiguous()
    vf = v.float().reshape(b * hk, t, d)
    kq = flush(kt, F.oracle_q(kt, cfg0["w_quantizer"])).transpose(1, 2).reshape(b, hk, t, d)
    return kq, flush(vf, F.oracle_q(vf, cfg1["w_quantizer"])).reshape(b, hk, t, d)


def _dense(k, v, cfg0, cfg1, pattern, capacity=96):
    from lqer_amd import QuantizedKVCache

    b, hk, t, d = k.shape
    cache = QuantizedKVCache(b, hk, d, cfg0, cfg1, k.dtype, k.device, capacity=capacity)
    cache.buf.zero_()  # (so that two caches compare byte for byte, the V rows no append writes included)
    at = 0
    for n in pattern:
        cache.append(k[:, :, at:at + n], v[:, :, at:at + n])
        at += n
    assert at == t == cache.length
    return cache


# (fp16 holds the ladders of the formats in F.FP16_IDS only)
KV_CASES = [pytest.param(p, t, dt, id=f"K{p[0]}w{p[1]}-V{p[2]}w{p[3]}-t{t}-{dt}") for p in KV_PAIRS for t in (37, 77) for dt in DTYPES
            if dt != "f16" or (p[0] in F.FP16_IDS and p[2] in F.FP16_IDS)]


@pytest.mark.parametrize("pair,t,dt", KV_CASES)
def test_kv_stored_values_and_chunked_bytes(pair, t, dt):
    """append in uneven steps, then dequantized() == the oracle's quantizer on K^T and V; the section bytes equal a one-shot append's."""
    from lqer_amd import kvcache

    fk, wk, fv, wv = pair
    dtype = DTYPES[dt]
    cfg0, cfg1 = _kv_cfgs(*pair)
    b, hk, d = 2, 2, 48
    k, v = _kv_ladder(fk, fv, dtype, b, hk, t, d, seed=200 + t)
    F.assert_covered(k.reshape(b * hk, t, d).transpose(1, 2).contiguous(), fk, cfg0["w_quantizer"], dtype)
    F.assert_covered(v.reshape(b * hk * t, d), fv, cfg1["w_quantizer"], dtype)
    want_k, want_v = _kv_oracle(k, v, cfg0, cfg1)
    steps = [5, 11, 1, 14, t - 31]
    chunked = _dense(k.to(DEV), v.to(DEV), cfg0, cfg1, steps)
    got_k, got_v = (x.cpu() for x in chunked.dequantized())
    assert torch.equal(got_k, want_k), f"K: {(got_k != want_k).sum().item()} of {want_k.numel()} differ"
    assert torch.equal(got_v, want_v), f"V: {(got_v != want_v).sum().item()} of {want_v.numel()} differ"
    once = _dense(k.to(DEV), v.to(DEV), cfg0, cfg1, [t])
    sections, _ = kvcache._sections(dtype, b, hk, chunked.capacity, d)
    z, blocks = b * hk, (t + 15) // 16
    for name, at, per_block in sections[:4]:
        row = (chunked.capacity // 16) * per_block
        a, o = (c.buf[at:at + z * row].view(z, row)[:, :blocks * per_block] for c in (chunked, once))
        assert torch.equal(a, o), f"{name}: {(a != o).sum().item()} bytes differ from the one-append cache"
    # the exponent bytes: the oracle's block exponent less emin; a zero block stores 0 clamped to the format's range (emin > 0: e3bm2)
    cap16, off = chunked.capacity // 16, {name: at for name, at, _ in sections}
    kt = k.float().reshape(z, t, d).transpose(1, 2).contiguous()
    for name, src, fid, c in (("k_exps", kt, fk, cfg0["w_quantizer"]), ("v_exps", v.float().reshape(z, t, d), fv, cfg1["w_quantizer"])):
        emin, emax = F.e_range(fid)
        _, _, e = F.oracle_q(src, c, decompose=True)
        blk, _ = O._blocks(src, c["block_size"], True)
        e = torch.where(blk.abs().amax(dim=-1) != 0, e, torch.full_like(e, min(max(0, emin), emax))) - emin
        got = chunked.buf[off[name]:off[name] + z * cap16 * d].cpu()
        if name == "k_exps":  # byte of (block of 16 keys kb, d) at kb D + d
            got, want = got.view(z, cap16, d)[:, :blocks], e.reshape(z, d, blocks).permute(0, 2, 1)
        else:                 # byte of (key 16 kb + tt, block db of 16 d) at (kb D / 16 + db) 16 + tt
            got = got.view(z, cap16, d // 16, 16).permute(0, 1, 3, 2).reshape(z, cap16 * 16, d // 16)[:, :t]
            want = e.reshape(z, t, d // 16)
        assert torch.equal(got.int(), want.int()), f"{name}: {(got.int() != want.int()).sum().item()} of {want.numel()} exponent bytes differ"


def _same_bits_inputs(quad, shape, mode, dtype, cfg0, cfg1):
    """q, k, v on the GPU.  The mask cases draw plain normal K / V at scale 3 / 1, which meet no clamp of e4, e5b20 or e8b120; the causal
    cases take K^T and V from the formats' ladders (asserted to reach every class the dtype holds), with q at 2^-10 so that the scores
    stay inside fp16: there the cache's reader meets exponent bytes at both clamps, and zero blocks."""
    b, h, hk, s, t, d = shape
    if mode != "causal":
        return tuple(x.to(DEV) for x in (A._randn((b, h, s, d), dtype, 10, 3.0), A._randn((b, hk, t, d), dtype, 11, 3.0), A._randn((b, hk, t, d), dtype, 12)))
    (_, _), (fk, _), _, (fv, _) = QUADS[quad]
    k, v = _kv_ladder(fk, fv, dtype, b, hk, t, d, seed=400 + t)
    F.assert_covered(k.reshape(b * hk, t, d).transpose(1, 2).contiguous(), fk, cfg0["w_quantizer"], dtype)
    F.assert_covered(v.reshape(b * hk * t, d), fv, cfg1["w_quantizer"], dtype)
    return (A._randn((b, h, s, d), dtype, 10, 2.0 ** -10)).to(DEV), k.to(DEV), v.to(DEV)


ATT_QUADS = ["narrowP-e3b6", "kv-e3bm2-e2", "all-w4", "mixed-8463"]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", ["mask", "causal"])
@pytest.mark.parametrize("shape", [(2, 4, 2, 5, 37, 48), (2, 8, 2, 8, 300, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("quad", ATT_QUADS)
def test_same_bits_as_the_raw_decode_kernel(quad, shape, mode, dt):
    from lqer_amd import attention_flexible, attention_flexible_cached

    b, h, hk, s, t, d = shape
    dtype = DTYPES[dt]
    cfg0, cfg1 = cfgs(quad)
    q, k, v = _same_bits_inputs(quad, shape, mode, dtype, cfg0, cfg1)
    mask = A._mask(mode, b, s, t, dtype)
    mask = None if mode == "causal" else mask.to(DEV)
    cache = _dense(k, v, cfg0, cfg1, [t - 1, 1], capacity=320)
    out, st = attention_flexible_cached(q, cache, d ** -0.5, attention_mask=mask, causal=mode == "causal", return_stats=True)
    want, want_st = attention_flexible(q, k, v, cfg0, cfg1, d ** -0.5, attention_mask=mask, causal=mode == "causal", return_stats=True, kernel="decode")
    assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), f"{(out != want).sum().item()} of {out.numel()} outputs differ"
    assert torch.equal(st.view(torch.uint8), want_st.view(torch.uint8)) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("mode", ["mask", "causal"])
@pytest.mark.parametrize("shape", [(2, 4, 2, 20, 37, 48), (1, 4, 2, 70, 150, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("quad", ATT_QUADS)
def test_same_bits_as_the_raw_prefill_kernel(quad, shape, mode, dt):
    from lqer_amd import attention_flexible, attention_flexible_cached

    b, h, hk, s, t, d = shape
    dtype = DTYPES[dt]
    cfg0, cfg1 = cfgs(quad)
    q, k, v = _same_bits_inputs(quad, shape, mode, dtype, cfg0, cfg1)
    mask = A._mask(mode, b, s, t, dtype)
    mask = None if mode == "causal" else mask.to(DEV)
    cache = _dense(k, v, cfg0, cfg1, [t - s, s], capacity=160)
    out, st = attention_flexible_cached(q, cache, d ** -0.5, attention_mask=mask, causal=mode == "causal", return_stats=True, kernel="prefill")
    want, want_st = attention_flexible(q, k, v, cfg0, cfg1, d ** -0.5, attention_mask=mask, causal=mode == "causal", return_stats=True, kernel="prefill")
    assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), f"{(out != want).sum().item()} of {out.numel()} outputs differ"
    assert torch.equal(st.view(torch.uint8), want_st.view(torch.uint8)) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("pair", KV_PAIRS[:6], ids=lambda p: f"K{p[0]}w{p[1]}-V{p[2]}w{p[3]}")
def test_paged_pool_equals_dense_per_sequence(pair, dt):
    """Two sequences of 37 and 77 keys in one pool: the gathered values are the oracle's, the decode attention over the pool gives the
    bits of the dense cache per sequence."""
    from lqer_amd import PagedKVCache, attention_flexible_cached, attention_flexible_paged

    fk, wk, fv, wv = pair
    dtype = DTYPES[dt]
    cfg0, cfg1 = _kv_cfgs(*pair)
    hk, h, d, lens = 2, 4, 48, (37, 77)
    raws = [_kv_ladder(fk, fv, dtype, 1, hk, n, d, seed=300 + n) for n in lens]
    for k, v in raws:
        F.assert_covered(k.reshape(hk, -1, d).transpose(1, 2).contiguous(), fk, cfg0["w_quantizer"], dtype)
        F.assert_covered(v.reshape(-1, d), fv, cfg1["w_quantizer"], dtype)
    pool = PagedKVCache(sum((n + 15) // 16 for n in lens), 2, hk, d, cfg0, cfg1, dtype, DEV, max_pages_per_seq=5)
    seqs = [pool.alloc() for _ in lens]
    for sq, (k, v), n in zip(seqs, raws, lens):  # uneven steps
        pool.append([sq], k[:, :, :21].to(DEV), v[:, :, :21].to(DEV))
        pool.append([sq], k[:, :, 21:].to(DEV), v[:, :, 21:].to(DEV))
    q = A._randn((2, h, 3, d), dtype, 7, 2.0).to(DEV)
    out, st = attention_flexible_paged(q, pool, seqs, d ** -0.5, causal=True, return_stats=True)
    for i, (sq, (k, v)) in enumerate(zip(seqs, raws)):
        want_k, want_v = _kv_oracle(k, v, cfg0, cfg1)
        got_k, got_v = (x.cpu() for x in pool.dequantized(sq))
        assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v), i
        dense = _dense(k.to(DEV), v.to(DEV), cfg0, cfg1, [k.shape[2]])
        want, want_st = attention_flexible_cached(q[i:i + 1], dense, d ** -0.5, causal=True, return_stats=True)
        assert torch.equal(out[i:i + 1].view(torch.uint8), want.view(torch.uint8)) and torch.equal(st[i:i + 1].view(torch.uint8), want_st.view(torch.uint8)), i

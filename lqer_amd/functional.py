"""Quantized attention matmuls - mirror of the reference's quantized_functions package for this path
(src/lqer/quantize/quantized_functions/matmul.py:12-37, __init__.py:3-21; call sites llama_decoder.py:263,294 and
opt_decoder.py:125,190):   product = matmul(x_quantizer(x), w_quantizer(y)).

Blocks run along the last dim of each operand, which for y is NOT the contraction dim (llama-7b.toml:110-126).  With the
templates' settings (block_fp, width <= 8, blocks of 16) the whole product is ONE fused HIP GEMM (lqer_matmul_q,
csrc/matmul_q.hip): x is quantized in the GEMM's load path - read from HBM once, no quantized copy -, y through a small bf16
image, bf16 MFMA with fp32 accumulation of exact products; 4-D [bsz, heads, ..] operands are folded into one batch dim.  Other
block lengths (16 n elements, or whole rows; no template uses them) and minifloat operands take the same product kernel behind the
library's standalone quantizer: that operand's bf16 image is written first and read as it is - the same bits.  Only operands whose
leading dims broadcast (no call site has them) run the quantizer kernels on both operands and hand the two quantized tensors to
torch.matmul / torch.bmm.  Quantizer settings outside what the kernels implement raise - there is no software fallback.
"""
from __future__ import annotations

from copy import deepcopy

import torch

import ctypes as C

from . import _lib, ops

MATMUL_MAP = {"matmul": torch.matmul, "bmm": torch.bmm}


def _quantize(t: torch.Tensor, cfg: dict) -> torch.Tensor:
    cfg = dict(cfg)
    name = cfg.get("name")
    if name == "passthrough":
        return t
    if name == "minifloat":  # elementwise: the standalone HIP quantizer
        ops._need_gpu(t)
        return ops.quantize_mxint(t, ops.make_qfmt(cfg), want=("deq",))["deq"].to(t.dtype)
    if name != "block_fp":
        raise NotImplementedError(f"lqer_amd.functional: quantizer {name!r} is not implemented on the HIP path")
    ops._need_gpu(t)
    fmt = ops.make_qfmt(cfg)
    if getattr(fmt, "act_tiles", None) is not None:
        # blocks that can span rows (incl. the quantizer's default lone [L], which the reference right-aligns to [1, S, L] on a 3-D operand,
        # quantizers/utils.py:56-66, 211-237): the HIP tile quantizer, as the reference blocks this very tensor (2-D / 3-D; else its error)
        if t.dim() not in (2, 3):
            raise RuntimeError(f"Unsupported x.ndim = {t.dim()}")  # (quantizers/utils.py:284)
        return ops.quantize_act_tiles(t, fmt)
    if fmt.block > 0 and fmt.block < t.shape[-1] and fmt.block % 16:
        raise NotImplementedError(f"lqer_amd.functional: block_size {cfg.get('block_size')} - the quantizer kernels take blocks of 16 n "
                                  "elements or whole rows along the last dim")
    return ops.quantize_mxint(t, fmt, want=("deq",))["deq"].to(t.dtype)


def _fused_fmt(cfg: dict):
    """The lqer_qfmt_t of a quantizer the library's product kernels cover (block_fp, width <= 8, blocks of 16 n elements or
    whole rows along the last dim: 16 runs fused in the load path, other lengths through the standalone quantizer's bf16
    image first - csrc/matmul_q.hip; minifloat operands likewise, through that quantizer's bf16 image), else None."""
    if cfg.get("name") == "minifloat":
        return ops.make_qfmt(cfg, "x")  # (raises on a format the HIP path refuses, as _quantize would)
    if cfg.get("name") != "block_fp" or int(cfg.get("width", 12)) > 8:
        return None
    try:
        fmt = ops.make_qfmt(cfg, "x")
    except NotImplementedError:
        return None
    if getattr(fmt, "act_tiles", None) is not None:
        return None  # (blocks that can span rows: the tile quantizer + the library product, _quantize above)
    return fmt if (fmt.block <= 0 or fmt.block % 16 == 0) else None


_MAX_GRID_Z = 65535  # the kernels put the batch on grid.z


@torch.no_grad()
def _matmul_fused(x: torch.Tensor, y: torch.Tensor, fx, fy) -> torch.Tensor:
    """x [.., S1, K] @ y [.., K, S2] (equal leading dims, or both 2-D) through lqer_matmul_q.  Leading dims are folded into
    one batch dim (the llama call sites hand over 4-D [bsz, heads, ...] operands, llama_decoder.py:263,294) - as a view
    where the strides allow, e.g. the transposed view of K in Q K^T -, and batches beyond the grid limit go in chunks."""
    lead = x.shape[:-2]
    squeeze = x.dim() == 2
    x3 = x[None] if squeeze else (x.flatten(0, -3) if x.dim() > 3 else x)
    y3 = y[None] if squeeze else (y.flatten(0, -3) if y.dim() > 3 else y)
    b, S1, K = x3.shape
    S2 = y3.shape[2]
    if x3.stride(2) != 1 or x3.stride(1) < K:
        x3 = x3.contiguous()
    if y3.stride(1) != 1 and y3.stride(2) != 1:  # (the kernel reads y dense along k - the transposed view of K - or along j)
        y3 = y3.contiguous()
    # an operand whose blocks are not 16 goes through the standalone quantizer first: evenly spaced rows over the batch, y dense along j
    x_pre, y_pre = fx.block != 16, fy.block != 16
    if x_pre and b > 1 and x3.stride(0) != S1 * x3.stride(1):
        x3 = x3.contiguous()
    if y_pre and (y3.stride(2) != 1 or (b > 1 and y3.stride(0) != K * y3.stride(1))):
        y3 = y3.contiguous()
    out = torch.empty(b, S1, S2, dtype=x.dtype, device=x.device)
    L = _lib.lib()
    with torch.cuda.device(x.device):
        for b0 in range(0, b, _MAX_GRID_Z):
            xb, yb, ob = x3[b0:b0 + _MAX_GRID_Z], y3[b0:b0 + _MAX_GRID_Z], out[b0:b0 + _MAX_GRID_Z]
            nb = xb.shape[0]
            nws = L.lqer_matmul_q_workspace_bytes_fmt(nb, S1, K, S2, C.byref(fx), C.byref(fy))
            ws = ops.workspace(x.device, max(nws, 16))
            ys = yb.stride()
            _lib.check(L.lqer_matmul_q(xb.data_ptr(), yb.data_ptr(), ob.data_ptr(), ops.dtype_code(x3), nb, S1, K, S2, xb.stride(0),
                                       xb.stride(1), ys[0], ys[1], ys[2], C.byref(fx), C.byref(fy), ws.data_ptr(), ws.numel(),
                                       ops._stream(x.device)),
                       "lqer_matmul_q")
    return out[0] if squeeze else out.reshape(*lead, S1, S2)


def generic_matmul_flexible(x: torch.Tensor, y: torch.Tensor, q_config: dict, style: str = "matmul") -> torch.Tensor:
    matmul = MATMUL_MAP[style]
    # q_config["default"] is evaluated eagerly, as in the reference (matmul.py:15-16)
    x_cfg = deepcopy(q_config.get("x_quantizer", q_config["default"]))
    w_cfg = deepcopy(q_config.get("w_quantizer", q_config["default"]))
    fx, fy = _fused_fmt(x_cfg), _fused_fmt(w_cfg)
    if (fx is not None and fy is not None and x.dtype == y.dtype and x.dtype in ops._DT and x.dim() == y.dim() and x.dim() >= 2
            and (style == "matmul" or x.dim() == 3)  # (torch.bmm takes 3-D operands only: anything else raises below, as there)
            and x.shape[-1] == y.shape[-2] and x.shape[:-2] == y.shape[:-2] and x.numel() > 0 and y.numel() > 0):
        ops._need_gpu(x, y)
        return _matmul_fused(x, y, fx, fy)
    return matmul(_quantize(x, x_cfg), _quantize(y, w_cfg))


def matmul_flexible(x, y, q_config):
    return generic_matmul_flexible(x, y, q_config, style="matmul")


def bmm_flexible(x, y, q_config):
    return generic_matmul_flexible(x, y, q_config, style="bmm")


# ---- fused attention (csrc/attn_q.hip: prefill; csrc/attn_decode.hip: up to 8 query rows, split over the keys) ----------------
ROUTE_FUSED, ROUTE_UNFUSED = "fused", "unfused"
KERNEL_PREFILL, KERNEL_DECODE = "prefill", "decode"
_ATTN_MAX_D = 128
_ATTN_MAX_T = 65535 * 64  # the image kernels put t / 64 on grid.y
_ATTN_DECODE_MAX_S = 8    # query rows per head the decode kernel takes (lqer_attention_q_decode refuses more)


def _attn_fmts(cfg0: dict, cfg1: dict):
    """The four lqer_qfmt_t (Q, K^T, P, V) when the fused kernel covers them - block_fp, width <= 8, blocks of 16 along the
    last dim, no tiles that span rows - else None."""
    fmts = []
    for cfg in (cfg0, cfg1):
        for key in ("x_quantizer", "w_quantizer"):
            c = cfg.get(key, cfg.get("default"))
            if c is None or c.get("name") != "block_fp":
                return None
            f = _fused_fmt(deepcopy(c))
            if f is None or f.kind != _lib.Q_MXINT or f.block != 16:
                return None
            fmts.append(f)
    return fmts


def _mask_ok(m, q, t: int) -> bool:
    """A mask the fused kernels read: additive, [b|1, h|1, s|1, t] of q's dtype on q's device, dense along t."""
    b, h, s, _ = q.shape
    return (m.dim() == 4 and m.dtype == q.dtype and m.device == q.device and m.shape[3] == t and (m.stride(3) == 1 or t == 1)
            and m.shape[0] in (1, b) and m.shape[1] in (1, h) and m.shape[2] in (1, s))


def _attention_route(q, k, v, cfg0, cfg1, attention_mask=None, causal=False):
    """(route tag, formats): which route attention_flexible takes for these operands."""
    if not (q.dim() == k.dim() == v.dim() == 4) or not (q.is_cuda and k.is_cuda and v.is_cuda):
        return ROUTE_UNFUSED, None
    b, h, s, d = q.shape
    hk, t = k.shape[1], k.shape[2]
    ok = (q.dtype == k.dtype == v.dtype and q.dtype in ops._DT and d % 16 == 0 and 0 < d <= _ATTN_MAX_D and s > 0 and 0 < t <= _ATTN_MAX_T and b > 0
          and not (causal and s > t)  # (rows without a visible key: the kernel gives them 0, the mask tensor a uniform row)
          and k.shape == v.shape and k.shape[0] == b and k.shape[3] == d and hk > 0 and h % hk == 0
          and b <= _MAX_GRID_Z and h <= _MAX_GRID_Z and b * hk <= _MAX_GRID_Z
          and q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1)
    if ok and attention_mask is not None:
        ok = not causal and _mask_ok(attention_mask, q, t)
    if not ok:
        return ROUTE_UNFUSED, None
    fmts = _attn_fmts(cfg0, cfg1)
    return (ROUTE_FUSED, fmts) if fmts is not None else (ROUTE_UNFUSED, None)


def _decode_covers(q) -> bool:
    """Operands of the fused route that the decode kernel takes as well (everything else it needs, the fused route needs too)."""
    return q.shape[2] <= _ATTN_DECODE_MAX_S


# The automatic rule follows the measurement of tools/attn_decode_bench.py (profiles/attn_decode.json: fp16, d = 128, whole calls of
# attention_flexible timed, 15 shapes), in terms of the K / V streams = batch x kv_heads and of t:
#   streams <= 64: the decode kernel won at every t measured from 512 to 32768 (32 streams; 64 streams at t = 2048, with and without
#                  grouped-query heads), by 1.07x to 10x; below 32 streams nothing else was ever in reach of it;
#   t <= 128 with 32 streams or more: the prefill kernel (43.5 against 43.9 us at 32 streams, 44.3 against 58.0 us at 256: one
#                  workgroup per head covers so few keys, and nothing is split);
#   streams > 64 and t > 128: the unfused route (128 streams, t = 2048: 113.2 against 115.1 us; 256 streams, t = 512 / 2048 / 8192:
#                  91.7 / 165.7 / 656.8 against 124.5 / 214.8 / 970.9 us) - the decode kernel streams K and V at about 1.3 TB/s, the two
#                  unfused products do better once there is enough of them.  Between 64 and 128 streams nothing is measured.
_ATTN_DECODE_MAX_STREAMS = 64
_ATTN_DECODE_SHORT_T, _ATTN_DECODE_SHORT_T_STREAMS = 128, 32


def _decode_rule(b: int, hk: int, t: int):
    """"decode", "prefill" or None (the unfused route) for s <= 8 query rows."""
    streams = b * hk
    if t <= _ATTN_DECODE_SHORT_T and streams >= _ATTN_DECODE_SHORT_T_STREAMS:
        return KERNEL_PREFILL
    if streams > _ATTN_DECODE_MAX_STREAMS:
        return None
    return KERNEL_DECODE


def _check_kernel_arg(kernel) -> None:
    if kernel not in (None, KERNEL_PREFILL, KERNEL_DECODE):
        raise ValueError(f"kernel {kernel!r}: None, 'prefill' or 'decode'")


def _check_layout_and_mask(who: str, out_layout, attention_mask, causal) -> None:
    if out_layout not in ("bhsd", "bshd"):
        raise ValueError(f"out_layout {out_layout!r}: 'bhsd' or 'bshd'")
    if attention_mask is not None and causal:
        raise ValueError(f"{who}: attention_mask and causal=True are two forms of one mask - pass one")


def _attention_kernel(q, k, v, cfg0, cfg1, attention_mask=None, causal=False, kernel=None):
    """(kernel name or None for the unfused route, formats).  kernel=None: up to 8 query rows take the decode kernel - or, where
    tools/attn_decode_bench.py measured another leg faster, that leg (_decode_rule) -, more take the prefill kernel;
    "prefill" / "decode" force one and raise where it does not apply."""
    _check_kernel_arg(kernel)
    route, fmts = _attention_route(q, k, v, cfg0, cfg1, attention_mask, causal)
    if route != ROUTE_FUSED:
        if kernel is not None:
            raise ValueError(f"attention_flexible: kernel={kernel!r} forced, but these operands take the unfused route (attention_flexible.route)")
        return None, None
    if kernel == KERNEL_DECODE and not _decode_covers(q):
        raise ValueError(f"attention_flexible: kernel='decode' takes up to {_ATTN_DECODE_MAX_S} query rows per head, got {q.shape[2]}")
    if kernel is None:
        kernel = _decode_rule(q.shape[0], k.shape[1], k.shape[2]) if _decode_covers(q) else KERNEL_PREFILL
        if kernel is None:
            return None, None
    return kernel, fmts


def _repeat_kv(t: torch.Tensor, n_rep: int) -> torch.Tensor:
    if n_rep == 1:
        return t
    b, h, s, d = t.shape
    return t[:, :, None, :, :].expand(b, h, n_rep, s, d).reshape(b, h * n_rep, s, d)


def unfused_attention(q, k, v, cfg0, cfg1, scaling, attention_mask=None, dropout=0.0, training=False):
    """The unfused sequence - the ONE body behind lqer_amd.attention.lqer_eager_attention_forward and every fall-back of
    attention_flexible: grouped-query K / V repeated, matmul_flexible, scale, mask add, fp32 softmax, cast, (dropout,) matmul_flexible.
    q [b, h, s, d], k / v [b, h_kv, t, d] -> out [b, h, s, d], weights [b, h, s, t]."""
    b, h, s, d = q.shape
    k, v = _repeat_kv(k, h // k.shape[1]), _repeat_kv(v, h // v.shape[1])
    t = k.shape[2]
    scores = matmul_flexible(q.reshape(b * h, s, d), k.reshape(b * h, t, d).transpose(1, 2), cfg0)
    w = scores.reshape(b, h, s, t) * scaling
    if attention_mask is not None:
        w = w + attention_mask
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    w = torch.nn.functional.dropout(w, p=dropout, training=training)
    out = matmul_flexible(w.reshape(b * h, s, t), v.reshape(b * h, t, d), cfg1)
    return out.reshape(b, h, s, d), w


def _causal_mask(s, t, dtype, device):
    """The additive tensor form of the causal rule, as eager_mask builds it: the dtype's most negative finite value where j > i + (t - s)."""
    i, j = torch.arange(s, device=device)[:, None], torch.arange(t, device=device)[None, :]
    return torch.zeros(s, t, dtype=dtype, device=device).masked_fill_(j > i + (t - s), torch.finfo(dtype).min)[None, None]


_I64X3 = C.c_int64 * 3


def _tri(t: torch.Tensor, bcast: bool = False):
    """The stride triple (elements over batch / head / row) of a 4-d tensor for the C ABI; bcast: 0 over a dim of size 1 (a mask's)."""
    st = t.stride()
    if bcast:
        sh = t.shape
        return _I64X3(0 if sh[0] == 1 else st[0], 0 if sh[1] == 1 else st[1], 0 if sh[2] == 1 else st[2])
    return _I64X3(st[0], st[1], st[2])


def _attention_outputs(q, out_layout: str, return_stats: bool):
    """(out, its [b, h, s, d] view, stats or None) for q [b, h, s, d]: out is [b, s, h, d] with "bshd", written through the view."""
    b, h, s, d = q.shape
    out = torch.empty((b, h, s, d) if out_layout == "bhsd" else (b, s, h, d), dtype=q.dtype, device=q.device)
    stats = torch.empty(b, h, s, 2, dtype=torch.float32, device=q.device) if return_stats else None
    return out, (out if out_layout == "bhsd" else out.transpose(1, 2)), stats


def _attention_call(name: str, q, *, kv=None, cache=None, mask, causal, out, stats, fmts, scaling, ws=None) -> None:
    """The C attention call `name` (one of the four: one argument list but for the K / V source) on q [b, h, s, d].  The source is
    kv = (k, v), tensors [b, h_kv, t, d], or cache = (buf, capacity, kv_heads, length) of a packed cache.  mask: the tensor or None;
    out: a [b, h, s, d] tensor or view; stats: [b, h, s, 2] fp32 or None; ws: a uint8 workspace, or None for the stream's at the size
    `name`_workspace_bytes asks."""
    b, h, s, d = q.shape
    m = mask
    if cache is None:
        k, v = kv
        hk, t = k.shape[1], k.shape[2]
        src, src_tri = (k.data_ptr(), v.data_ptr()), (_tri(k), _tri(v))
    else:
        buf, capacity, hk, t = cache
        src, src_tri = (buf.data_ptr(), buf.numel(), capacity), ()
    L = _lib.lib()
    with torch.cuda.device(q.device):
        if ws is None:
            ws = ops.workspace(q.device, max(getattr(L, name + "_workspace_bytes")(b, h, hk, s, t, d), 16))
        _lib.check(getattr(L, name)(q.data_ptr(), *src, m.data_ptr() if m is not None else None, out.data_ptr(),
                                    stats.data_ptr() if stats is not None else None, ops.dtype_code(q), b, h, hk, s, t, d, _tri(q), *src_tri,
                                    _tri(m, bcast=True) if m is not None else None, _tri(out), float(scaling), int(bool(causal)),
                                    C.byref(fmts[0]), C.byref(fmts[1]), C.byref(fmts[2]), C.byref(fmts[3]), ws.data_ptr(), ws.numel(),
                                    ops._stream(q.device)),
                   name)


@torch.no_grad()
def attention_flexible(q, k, v, cfg0, cfg1, scaling, attention_mask=None, causal=False, out_layout="bhsd", return_stats=False,
                       return_route=False, kernel=None):
    """softmax(Q_x0(q) Q_w0(k^T) * scaling + mask) -> Q_x1 -> @ Q_w1(v) on q [b, h, s, d], k / v [b, h_kv, t, d] (grouped-query heads
    through the head mapping): lqer_eager_attention_forward's computation, every intermediate rounded to the operands' dtype where
    that route materialises it.  With the templates' quantizers (block_fp, width <= 8, blocks of 16), d a multiple of 16 up to 128
    and rows dense along d it is ONE fused HIP kernel behind two small image kernels (lqer_attention_q, csrc/attn_q.hip) and the
    scores stay on the chip; anything else runs the unfused sequence with that route's results - never an approximation.
    With up to 8 query rows (a decode step against a KV cache) the fused route runs the kernel that is split over the keys instead
    (lqer_attention_q_decode, csrc/attn_decode.hip: K and V read once, no images); `kernel` = "prefill" / "decode" forces one of the
    two (ValueError where it does not cover the operands), None chooses; attention_flexible.kernel(...) tells which.
    `attention_mask`: additive, broadcastable [b|1, h|1, s|1, t] of q's dtype; `causal`: key j visible to query i iff j <= i + (t - s)
    (the tensor form of that rule: with s > t, where early rows see no key at all, the unfused sequence runs on that tensor).
    `out_layout`: "bhsd" or "bshd" (what the HuggingFace attention interface returns, written directly).  Returns out, then
    `stats` [b, h, s, 2] fp32 = {row max of the masked scores, row sum of exp(score - max)} with return_stats (fused route only,
    else None), then the route tag with return_route."""
    _check_layout_and_mask("attention_flexible", out_layout, attention_mask, causal)
    kern, fmts = _attention_kernel(q, k, v, cfg0, cfg1, attention_mask, causal, kernel)  # (validates `kernel`; CPU tensors: no kernel)
    ops._need_gpu(q, k, v, attention_mask)
    route = ROUTE_FUSED if kern is not None else ROUTE_UNFUSED
    stats = None
    if route == ROUTE_FUSED:
        out, ob, stats = _attention_outputs(q, out_layout, return_stats)
        _attention_call("lqer_attention_q_decode" if kern == KERNEL_DECODE else "lqer_attention_q", q, kv=(k, v), mask=attention_mask, causal=causal,
                        out=ob, stats=stats, fmts=fmts, scaling=scaling)
    else:
        if causal:
            attention_mask = _causal_mask(q.shape[2], k.shape[2], q.dtype, q.device)
        out, _ = unfused_attention(q, k, v, cfg0, cfg1, scaling, attention_mask)
        if out_layout == "bshd":
            out = out.transpose(1, 2).contiguous()
    res = (out,)
    if return_stats:
        res += (stats,)
    if return_route:
        res += (route,)
    return res[0] if len(res) == 1 else res


def _route_tag(q, k, v, cfg0, cfg1, attention_mask=None, causal=False) -> str:
    """The tag attention_flexible returns with return_route for these operands (kernel=None)."""
    return ROUTE_FUSED if _attention_kernel(q, k, v, cfg0, cfg1, attention_mask, causal)[0] is not None else ROUTE_UNFUSED


def _kernel_tag(q, k, v, cfg0, cfg1, attention_mask=None, causal=False):
    """"decode", "prefill", or None for the unfused route: what attention_flexible runs for these operands with kernel=None."""
    return _attention_kernel(q, k, v, cfg0, cfg1, attention_mask, causal)[0]


attention_flexible.route = _route_tag
attention_flexible.kernel = _kernel_tag


QUANTIZED_FUNCTION_MAP = {"matmul": {"flexible": matmul_flexible}, "bmm": {"flexible": bmm_flexible}}


def get_quantized_func(op: str, q_config: dict):
    assert op in QUANTIZED_FUNCTION_MAP, f"Unsupported quantized op: {op}"
    assert q_config["name"] in QUANTIZED_FUNCTION_MAP[op], f"Unsupported quantized config: {q_config}"
    return QUANTIZED_FUNCTION_MAP[op][q_config["name"]]

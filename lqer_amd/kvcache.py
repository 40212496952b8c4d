"""A packed MXINT KV cache for the fused quantized attention (include/lqer_hip.h "packed KV cache"; csrc/kv_cache.hip writes it,
csrc/attn_decode.hip reads it; for more than 8 query rows csrc/kv_cache.hip turns it - the dense cache or the paged pool - into the
prefill kernel's two images).

The decode kernel quantizes the whole K (blocks of 16 along t) and V (blocks of 16 along d) in every step, with the results of
the step before.  The cache keeps the quantizer's output instead of the raw tensors - a one-byte code per element, a one-byte
exponent per block - and `attention_flexible_cached` multiplies that: the same bits as `attention_flexible(kernel="decode")` on the
raw K and V, from 2 d (1 + 1/16) bytes per token and kv head instead of 2 d itemsize.  With kernel="prefill" it takes any number of
query rows - a second prompt, a prompt fed in chunks - and gives the bits of `attention_flexible(kernel="prefill")`.  The raw values are
gone once appended, so nothing here falls back: what the kernels do not cover raises."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .functional import (KERNEL_DECODE, KERNEL_PREFILL, _ATTN_DECODE_MAX_S, _ATTN_MAX_D, _ATTN_MAX_T, _MAX_GRID_Z, _attention_call, _attention_outputs,
                         _attn_fmts, _check_kernel_arg, _check_layout_and_mask, _mask_ok, _tri)


def cache_bytes(dtype: torch.dtype, batch: int, kv_heads: int, capacity: int, head_dim: int) -> int:
    return _lib.lib().lqer_kv_cache_bytes(ops._DT[dtype], batch, kv_heads, capacity, head_dim)


def _sections(dtype: torch.dtype, batch: int, kv_heads: int, capacity: int, head_dim: int):
    """[(name, byte offset, bytes per (batch, kv head) and block of 16 keys - None for the staging rows, copied whole)] of the header's
    layout, and the total."""
    up = lambda v: (v + 255) // 256 * 256
    cap, z = (capacity + 15) // 16 * 16, batch * kv_heads
    codes, exps = up(z * cap * head_dim), up(z * (cap // 16) * head_dim)
    stage = up(z * 16 * head_dim * torch.empty((), dtype=dtype).element_size())
    out, at = [], 0
    for name, size, per_block in (("k_codes", codes, 16 * head_dim), ("k_exps", exps, head_dim), ("v_codes", codes, 16 * head_dim),
                                  ("v_exps", exps, head_dim), ("k_stage", stage, None)):
        out.append((name, at, per_block))
        at += size
    return out, at


@torch.no_grad()
def append_packed(buf: torch.Tensor, k: torch.Tensor, v: torch.Tensor, length: int, capacity: int, k_fmt, v_fmt) -> None:
    """lqer_kv_cache_append on a caller's buffer: k / v [batch, kv_heads, n, d] become keys length .. length + n - 1."""
    ops._need_gpu(buf, k, v)
    if k.dim() != 4 or k.shape != v.shape or k.dtype != v.dtype:
        raise ValueError(f"append: k {tuple(k.shape)} {k.dtype} and v {tuple(v.shape)} {v.dtype} must be equal-shaped [batch, kv_heads, n, d]")
    if k.stride(3) != 1:
        k = k.contiguous()
    if v.stride(3) != 1:
        v = v.contiguous()
    b, hk, n, d = k.shape
    with torch.cuda.device(k.device):
        _lib.check(_lib.lib().lqer_kv_cache_append(buf.data_ptr(), buf.numel(), k.data_ptr(), v.data_ptr(), _tri(k), _tri(v), ops.dtype_code(k), b, hk,
                                                   capacity, d, length, n, C.byref(k_fmt), C.byref(v_fmt), ops._stream(k.device)),
                   "lqer_kv_cache_append")


@torch.no_grad()
def unpack_packed(buf: torch.Tensor, dtype: torch.dtype, batch: int, kv_heads: int, capacity: int, head_dim: int, length: int, k_fmt, v_fmt):
    """The dequantized K and V [batch, kv_heads, length, d] as fp32 (lqer_kv_cache_unpack, a test hook)."""
    ops._need_gpu(buf)
    kf = torch.empty(batch, kv_heads, length, head_dim, dtype=torch.float32, device=buf.device)
    vf = torch.empty_like(kf)
    with torch.cuda.device(buf.device):
        _lib.check(_lib.lib().lqer_kv_cache_unpack(buf.data_ptr(), buf.numel(), ops._DT[dtype], batch, kv_heads, capacity, head_dim, length,
                                                   C.byref(k_fmt), C.byref(v_fmt), kf.data_ptr(), vf.data_ptr(), ops._stream(buf.device)),
                   "lqer_kv_cache_unpack")
    return kf, vf


@torch.no_grad()
def attend_packed(q, buf, kv_heads, capacity, length, fmts, scaling, attention_mask=None, causal=False, out=None, stats=None, ws=None):
    """lqer_attention_q_decode_kv on a caller's buffer.  q [b, h, s, d]; out: a [b, h, s, d] tensor or view (any strides over b, h, s);
    stats: [b, h, s, 2] fp32 or None; ws: a uint8 workspace or None (the stream's)."""
    _attention_call("lqer_attention_q_decode_kv", q, cache=(buf, capacity, kv_heads, length), mask=attention_mask, causal=causal, out=out, stats=stats,
                    fmts=fmts, scaling=scaling, ws=ws)


@torch.no_grad()
def prefill_packed(q, buf, kv_heads, capacity, length, fmts, scaling, attention_mask=None, causal=False, out=None, stats=None, ws=None):
    """lqer_attention_q_kv on a caller's buffer: attend_packed's arguments, any number of query rows."""
    _attention_call("lqer_attention_q_kv", q, cache=(buf, capacity, kv_heads, length), mask=attention_mask, causal=causal, out=out, stats=stats,
                    fmts=fmts, scaling=scaling, ws=ws)


def _check_covers(who: str, cfg0: dict, cfg1: dict, head_dim: int, dtype: torch.dtype) -> None:
    if not QuantizedKVCache.covers(cfg0, cfg1, head_dim, dtype):
        raise NotImplementedError(f"{who}: head_dim {head_dim}, dtype {dtype} or the quantizers of these configs are outside the "
                                  "packed cache (block_fp of width <= 8 with blocks of 16, head dims that are multiples of 16 up to 128, "
                                  "fp32 / fp16 / bf16) - and a cache without the raw values has no other route")


class QuantizedKVCache:
    """K and V of one attention layer as the codes and block exponents of the layer's two matmul configs (cfg0: Q K^T, cfg1: P V).

    .append(k, v)   k / v [batch, kv_heads, n, head_dim] of `dtype`, any n >= 1; grows by doubling when the capacity is passed
    .length         cached tokens;  .capacity  tokens the buffer holds;  .nbytes  bytes of the buffer
    .reset()        length 0 (the buffer needs no clearing: nothing depends on rows beyond the length)
    .dequantized()  (K, V) [batch, kv_heads, length, head_dim] fp32 - the quantizers' outputs, for tests"""

    @staticmethod
    def covers(cfg0: dict, cfg1: dict, head_dim: int, dtype: torch.dtype) -> bool:
        """Whether the packed cache and its kernel take these formats (block_fp, width <= 8, blocks of 16 - all four quantizers, since the
        attention over the cache is the fused decode kernel), this head dim (a multiple of 16 up to 128) and this dtype."""
        return (_attn_fmts(cfg0, cfg1) is not None and isinstance(head_dim, int) and 0 < head_dim <= _ATTN_MAX_D and head_dim % 16 == 0
                and dtype in ops._DT)

    def __init__(self, batch: int, kv_heads: int, head_dim: int, cfg0: dict, cfg1: dict, dtype: torch.dtype, device, capacity: int = 256):
        _check_covers("QuantizedKVCache", cfg0, cfg1, head_dim, dtype)
        if batch < 1 or kv_heads < 1 or capacity < 1 or batch > _MAX_GRID_Z or kv_heads > _MAX_GRID_Z:
            raise ValueError(f"QuantizedKVCache: batch {batch}, kv_heads {kv_heads}, capacity {capacity}")
        self.batch, self.kv_heads, self.head_dim, self.dtype, self.device = batch, kv_heads, head_dim, dtype, torch.device(device)
        self.cfg0, self.cfg1 = cfg0, cfg1
        self.fmts = _attn_fmts(cfg0, cfg1)  # Q, K^T, P, V
        self.length = 0
        self.capacity = (capacity + 15) // 16 * 16
        self.buf = self._alloc(self.capacity)

    def _alloc(self, capacity: int, batch=None) -> torch.Tensor:
        return torch.empty(cache_bytes(self.dtype, batch or self.batch, self.kv_heads, capacity, self.head_dim), dtype=torch.uint8, device=self.device)

    @property
    def nbytes(self) -> int:
        return self.buf.numel()

    def reset(self) -> None:
        self.length = 0

    def _grow(self, need: int) -> None:
        cap = self.capacity
        while cap < need:
            cap *= 2
        self.buf, self.capacity = self._moved(self.batch, cap), cap

    def _moved(self, new_batch: int, new_capacity: int, idx=None) -> torch.Tensor:
        """A new buffer for new_batch rows of new_capacity keys with what lives in this one: both as [batch, kv_heads, row] per section,
        the live blocks of the four code and exponent sections and the staging rows (one size at every capacity) - one copy each, of
        the batch rows `idx` (an int64 tensor on the device) where given."""
        new = self._alloc(new_capacity, new_batch)
        hk = self.kv_heads
        old_s, _ = _sections(self.dtype, self.batch, hk, self.capacity, self.head_dim)
        new_s, _ = _sections(self.dtype, new_batch, hk, new_capacity, self.head_dim)
        stage, blocks = 16 * self.head_dim * torch.empty((), dtype=self.dtype).element_size(), (self.length + 15) // 16
        for (_, o_at, per_block), (_, n_at, _) in zip(old_s, new_s):
            o_row, n_row = (stage, stage) if per_block is None else ((self.capacity // 16) * per_block, (new_capacity // 16) * per_block)
            live = stage if per_block is None else blocks * per_block
            if live:
                src = self.buf[o_at:o_at + self.batch * hk * o_row].view(self.batch, hk, o_row)[:, :, :live]
                new[n_at:n_at + new_batch * hk * n_row].view(new_batch, hk, n_row)[:, :, :live].copy_(src if idx is None else src.index_select(0, idx))
        return new

    @torch.no_grad()
    def append(self, k: torch.Tensor, v: torch.Tensor) -> None:
        want = (self.batch, self.kv_heads, self.head_dim)
        if k.dim() != 4 or (k.shape[0], k.shape[1], k.shape[3]) != want or k.shape != v.shape or k.dtype != self.dtype or v.dtype != self.dtype:
            raise ValueError(f"QuantizedKVCache.append: k {tuple(k.shape)} {k.dtype} / v {tuple(v.shape)} {v.dtype} for a cache of "
                             f"[{self.batch}, {self.kv_heads}, n, {self.head_dim}] {self.dtype}")
        n = k.shape[2]
        if n == 0:
            return
        if self.length + n > self.capacity:
            self._grow(self.length + n)
        append_packed(self.buf, k, v, self.length, self.capacity, self.fmts[1], self.fmts[3])
        self.length += n

    def dequantized(self):
        return unpack_packed(self.buf, self.dtype, self.batch, self.kv_heads, self.capacity, self.head_dim, self.length, self.fmts[1], self.fmts[3])

    @torch.no_grad()
    def select(self, indices) -> None:
        """Gather along the batch: row i becomes the old row indices[i] - a beam search's reorder, a repeat for several samples of one
        prompt, a subset; the batch may grow or shrink.  Out of place, as _grow: a new buffer of the same capacity takes the live
        blocks of the four code and exponent sections and the staging rows of every kv head of the selected rows, bytes as they are
        (torch's index_select - no kernel of the library), so row i then appends and attends with the bits old row indices[i] had."""
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
        if idx.numel() < 1 or idx.numel() > _MAX_GRID_Z or int(idx.min()) < 0 or int(idx.max()) >= self.batch:
            raise ValueError(f"QuantizedKVCache.select: indices {idx.tolist()} for a batch of {self.batch}")
        idx = idx.to(self.device)
        self.buf, self.batch = self._moved(idx.numel(), self.capacity, idx), idx.numel()


@torch.no_grad()
def attention_flexible_cached(q, cache: QuantizedKVCache, scaling, attention_mask=None, causal=False, out_layout="bhsd", return_stats=False,
                              kernel=None):
    """attention_flexible(q, K, V, cache.cfg0, cache.cfg1, scaling, ..., kernel="decode") for the K and V appended to `cache`, bit for
    bit, without K and V: lqer_attention_q_decode_kv reads the cache's codes.  q [b, h, s, d] with s <= 8 (ValueError beyond: a prefill
    attends over its own raw K and V with attention_flexible and then appends); masks, `out_layout` and `return_stats` as there.
    kernel="prefill" takes any s >= 1 - a second prompt or a chunk of a long one on a non-empty cache - and gives the bits of
    attention_flexible(..., kernel="prefill"): lqer_attention_q_kv writes the prefill kernel's two images from the codes.  None and
    "decode" are the decode kernel.  Operands the kernels do not take raise ValueError - there is no other route to the cached values."""
    _check_kernel_arg(kernel)
    prefill = kernel == KERNEL_PREFILL
    _check_layout_and_mask("attention_flexible_cached", out_layout, attention_mask, causal)
    ops._need_gpu(q, attention_mask)
    if q.dim() != 4:
        raise ValueError(f"attention_flexible_cached: q {tuple(q.shape)} is not [b, h, s, d]")
    b, h, s, d = q.shape
    t = cache.length
    if not prefill and s > _ATTN_DECODE_MAX_S:
        raise ValueError(f"attention_flexible_cached: {s} query rows per head - the kernel over the packed cache takes up to {_ATTN_DECODE_MAX_S}")
    if (q.dtype != cache.dtype or q.device != cache.buf.device or b != cache.batch or d != cache.head_dim or h % cache.kv_heads or s < 1 or t < 1
            or h > _MAX_GRID_Z or (causal and s > t) or (prefill and (t > _ATTN_MAX_T or b * cache.kv_heads > _MAX_GRID_Z))):
        raise ValueError(f"attention_flexible_cached: q {tuple(q.shape)} {q.dtype} against a cache of {t} keys [{cache.batch}, {cache.kv_heads}, "
                         f"{cache.head_dim}] {cache.dtype}" + (" (causal with more query rows than keys)" if causal and s > t else ""))
    m = attention_mask
    if m is not None and not _mask_ok(m, q, t):
        raise ValueError(f"attention_flexible_cached: mask {tuple(m.shape)} {m.dtype} - additive, [b|1, h|1, s|1, {t}] of q's dtype, dense along t")
    if q.stride(3) != 1:
        q = q.contiguous()
    out, ob, stats = _attention_outputs(q, out_layout, return_stats)
    (prefill_packed if prefill else attend_packed)(q, cache.buf, cache.kv_heads, cache.capacity, t, cache.fmts, scaling, m, causal, ob, stats)
    return (out, stats) if return_stats else out


# ---- the paged pool (include/lqer_hip.h "paged KV pool"): pages of 16 keys, per-sequence lengths in a decode batch ------------------
PAGE_KEYS = 16


def _pair(t: torch.Tensor):
    """The stride pair (elements over token / head) of a packed [total, heads, d] tensor for the C ABI's calls with per-sequence counts."""
    return (C.c_int64 * 2)(t.stride(0), t.stride(1))


def pool_bytes(dtype: torch.dtype, pages: int, slots: int, kv_heads: int, head_dim: int, k_fmt=None, v_fmt=None) -> int:
    """lqer_kv_pool_bytes, or - with the pool's K and V formats, either of which may name nibble codes (ops.nibble_qfmt) -
    lqer_kv_pool_bytes_fmt."""
    if k_fmt is None and v_fmt is None:
        return _lib.lib().lqer_kv_pool_bytes(ops._DT[dtype], pages, slots, kv_heads, head_dim)
    return _lib.lib().lqer_kv_pool_bytes_fmt(ops._DT[dtype], pages, slots, kv_heads, head_dim, C.byref(k_fmt), C.byref(v_fmt))


def _code_bits(code_bits, fmts):
    """PagedKVCache's code_bits -> (K bits, V bits), each 8 (a byte per code) or 4 (a nibble): None or 8 - bytes for both; 4 - nibbles
    for both; a pair - K and V on their own.  ValueError for anything else, and for 4 on an operand whose config is wider than 4 bits."""
    pair = (code_bits, code_bits) if code_bits is None or isinstance(code_bits, int) else tuple(code_bits)
    if len(pair) != 2 or any(isinstance(b, bool) or b not in (None, 4, 8) for b in pair):
        raise ValueError(f"PagedKVCache: code_bits {code_bits!r} - None, 8, 4 or a pair (k_bits, v_bits) of those")
    pair = tuple(8 if b is None else b for b in pair)
    for name, bits, f in zip(("K", "V"), pair, (fmts[1], fmts[3])):
        if bits == 4 and f.width > 4:
            raise ValueError(f"PagedKVCache: code_bits 4 for {name}, whose config is block_fp of width {f.width} - a nibble holds a sign and a "
                             "magnitude of at most 7: widths 2..4")
    return pair


@torch.no_grad()
def pool_copy(src: torch.Tensor, src_pages: int, src_slots: int, dst: torch.Tensor, dst_pages: int, dst_slots: int, dtype: torch.dtype,
              kv_heads: int, head_dim: int, ids: torch.Tensor, n_pages: int, n_slots: int, k_fmt=None, v_fmt=None) -> None:
    """lqer_kv_pool_copy on two pool buffers of the device: `ids`, an int32 tensor there, holds the source page ids, the destination page
    ids (n_pages each), the source slot ids and the destination slot ids (n_slots each) one behind the other.  k_fmt / v_fmt: the pools'
    K and V formats where a code section holds nibbles, else none."""
    ops._need_gpu(src, dst, ids)
    if ids.dtype != torch.int32 or not ids.is_contiguous() or ids.numel() != 2 * (n_pages + n_slots) or ids.device != dst.device or src.device != dst.device:
        raise ValueError(f"pool_copy: ids {tuple(ids.shape)} {ids.dtype} on {ids.device} for {n_pages} page pairs and {n_slots} slot pairs of pools "
                         f"on {src.device} / {dst.device}")
    at = [ids.data_ptr() + 4 * x for x in (0, n_pages, 2 * n_pages, 2 * n_pages + n_slots)]
    fmts = (None, None) if k_fmt is None and v_fmt is None else (C.byref(k_fmt), C.byref(v_fmt))
    with torch.cuda.device(dst.device):
        _lib.check(_lib.lib().lqer_kv_pool_copy(src.data_ptr(), src.numel(), src_pages, src_slots, dst.data_ptr(), dst.numel(), dst_pages, dst_slots,
                                                ops._DT[dtype], kv_heads, head_dim, at[0], at[1], n_pages, at[2], at[3], n_slots, *fmts,
                                                ops._stream(dst.device)),
                   "lqer_kv_pool_copy")


class KVPoolImage:
    """Sequences taken out of a PagedKVCache (export, swap_out): a small pool in the library's own layout - `pages` pages, the distinct
    pages of the sequences, and `slots` slots, one per sequence - with the books that say which pages make which sequence.  The bytes
    are the pool's as they are, so nibble codes, released pages under a window and pages shared between forks need no special case.

    .buf        uint8, pool layout (lqer_kv_pool_bytes(_fmt) of pages x slots; a pool has at least one page, so an image of empty
                sequences holds one that nothing names), on the device or in pinned host memory
    .books      PageTable.export's data, the pages renumbered 0 .. pages - 1: the image's own
    .signature  ints: dtype, kv_heads, head_dim, the K and V format fields, code_bits, window, max_query_rows - what adopt() compares
    .ready      a torch event recorded after the last copy that wrote buf (None once loaded from a state dict);  .synchronize() waits
    .nbytes;  .lengths  the sequences' lengths
    .state_dict() / KVPoolImage.from_state_dict(d): tensors and ints only - torch.save / torch.load work."""

    def __init__(self, buf: torch.Tensor, pages: int, books: dict, signature, ready=None):
        self.buf, self.pages, self.books, self.signature, self.ready = buf, pages, books, tuple(int(x) for x in signature), ready

    slots = property(lambda self: len(self.books["seqs"]))
    nbytes = property(lambda self: self.buf.numel())
    lengths = property(lambda self: [s[0] for s in self.books["seqs"]])

    def synchronize(self) -> None:
        if self.ready is not None:
            self.ready.synchronize()

    def state_dict(self) -> dict:
        self.synchronize()
        seqs = self.books["seqs"]
        return {"buf": self.buf.cpu(), "pages": self.pages, "signature": torch.tensor(self.signature, dtype=torch.int64),
                "lengths": torch.tensor([s[0] for s in seqs], dtype=torch.int64), "released": torch.tensor([s[1] for s in seqs], dtype=torch.int64),
                "rows": torch.tensor([p for s in seqs for p in s[2]], dtype=torch.int32)}

    @classmethod
    def from_state_dict(cls, d: dict) -> "KVPoolImage":
        rows, seqs, at = d["rows"].tolist(), [], 0
        for length, gone in zip(d["lengths"].tolist(), d["released"].tolist()):
            n = (length + PAGE_KEYS - 1) // PAGE_KEYS
            seqs.append((length, gone, rows[at:at + n]))
            at += n
        named = {p for _, gone, row in seqs for p in row[gone:]}
        if at != len(rows) or named != set(range(len(named))) or d["buf"].dtype != torch.uint8:
            raise ValueError("KVPoolImage.from_state_dict: the rows do not fit the lengths, or the buffer is not uint8")
        return cls(d["buf"], int(d["pages"]), {"pages": list(range(len(named))), "seqs": seqs}, d["signature"].tolist())


class PageTable:
    """The page allocator and the host mirror of the block table and the lengths: plain host state, no torch device in it.

    A sequence id is handed out once and never again, so a freed id stays refused; it maps to a SLOT (a row of the table, a set of
    staging rows), and slots and pages are reused.  `reserve` is all or nothing: it validates every addressed sequence and counts
    the pages of the whole call before it takes one.

    A page has a count of owners.  `fork` gives a new sequence the FULL pages of its parent by reference - a full page is never
    written again, so it needs no copy - and a page of its own for the open block; `free` hands a page back when its last owner
    goes.  A sequence that was never forked owns every one of its pages alone, and its books are what they were without the counts.

    `release(seq, before_key)` lets a sequence FORGET its oldest keys (a sliding window): it stops owning the leading pages that lie
    wholly below the key, and `released[slot]` counts them.  The row stays indexed by absolute key / 16: the released entries keep
    their old page ids - stale, but valid indices that nothing reads - and `pages_of` still counts entries from the row's start, so
    the pages a sequence holds are entries released .. pages_of - 1, and a row still needs room for the sequence's whole length.
    Indexing the row as a ring, so that it could be as short as the window, is not done here."""

    def __init__(self, num_pages: int, max_seqs: int, max_pages_per_seq=None):
        if max_pages_per_seq is None:
            max_pages_per_seq = num_pages
        if num_pages < 1 or max_seqs < 1 or max_pages_per_seq < 1:
            raise ValueError(f"PageTable: num_pages {num_pages}, max_seqs {max_seqs}, max_pages_per_seq {max_pages_per_seq}")
        self.num_pages, self.max_seqs, self.max_pages_per_seq = num_pages, max_seqs, max_pages_per_seq
        self._free_pages = list(range(num_pages - 1, -1, -1))  # a stack: the page freed last is taken first
        self._free_slots = list(range(max_seqs - 1, -1, -1))
        self._slot = {}                                        # live seq -> slot
        self._next_seq = 0
        self.table = [[0] * max_pages_per_seq for _ in range(max_seqs)]  # [slot][i]: the page of keys 16 i .. 16 i + 15
        self.pages_of = [0] * max_seqs                                   # entries of a slot's row in use, from the row's start
        self.released = [0] * max_seqs                                   # ... of which the leading ones are no longer its pages
        self.lengths = [0] * max_seqs                                    # [slot]
        self._owners = np.zeros(num_pages, dtype=np.int32)               # [page]: the live sequences whose rows name it

    @property
    def pages_free(self) -> int:
        return len(self._free_pages)

    @property
    def pages_shared(self) -> int:
        """Pages with more than one owner."""
        return int((self._owners > 1).sum())

    @property
    def max_len(self) -> int:
        """The bound handed to the library with every call: what the table's rows have room for, whatever the lengths are."""
        return PAGE_KEYS * self.max_pages_per_seq

    def alloc(self) -> int:
        if not self._free_slots:
            raise RuntimeError(f"PagedKVCache: all {self.max_seqs} sequence slots are live")
        seq, self._next_seq = self._next_seq, self._next_seq + 1
        slot = self._free_slots.pop()
        self._slot[seq] = slot
        self.pages_of[slot] = self.lengths[slot] = self.released[slot] = 0
        return seq

    def slot(self, seq: int) -> int:
        try:
            return self._slot[seq]
        except (KeyError, TypeError):
            raise KeyError(f"PagedKVCache: sequence {seq!r} is unknown or already freed") from None

    def free(self, seq: int) -> None:
        slot = self.slot(seq)
        del self._slot[seq]
        row = self.table[slot]
        if self.pages_of[slot] > self.released[slot]:
            pages = np.array(row[self.released[slot]:self.pages_of[slot]][::-1])  # the last page first: the order pages have always gone back in
            self._owners[pages] -= 1
            self._free_pages.extend(pages[self._owners[pages] == 0].tolist())  # (those whose last owner this was)
        self.pages_of[slot] = self.lengths[slot] = self.released[slot] = 0
        self._free_slots.append(slot)

    def length(self, seq: int) -> int:
        return self.lengths[self.slot(seq)]

    def pages_held(self, seq: int) -> int:
        """The pages the sequence owns, alone or shared: its row's entries minus the released ones."""
        slot = self.slot(seq)
        return self.pages_of[slot] - self.released[slot]

    def release(self, seq: int, before_key: int) -> list:
        """The sequence gives up its pages that lie wholly below key `before_key` (page i: keys 16 i .. 16 i + 15, so i <
        before_key // 16) - full pages only, never the open block.  A page goes back to the free stack when its last owner goes
        (forks share pages); returns the pages that did, in the order they went.  The row keeps the entries; a smaller or
        repeated `before_key` changes nothing.  unrelease() undoes the call."""
        slot = self.slot(seq)
        first, upto = self.released[slot], min(before_key // PAGE_KEYS, self.lengths[slot] // PAGE_KEYS)
        if upto <= first:
            return []
        pages = np.array(self.table[slot][first:upto])
        self._owners[pages] -= 1
        freed = pages[self._owners[pages] == 0].tolist()
        self._free_pages.extend(freed)
        self.released[slot] = upto
        return freed

    def unrelease(self, seq: int, first: int, freed: list) -> None:
        """Undo the release() that took released[slot] from `first` to its present value and returned `freed`, with no page taken
        or handed back since (or every such step undone): the books as they were, the free stack in its order."""
        slot = self.slot(seq)
        if freed:
            assert self._free_pages[-len(freed):] == freed
            del self._free_pages[-len(freed):]
        if self.released[slot] > first:
            self._owners[np.array(self.table[slot][first:self.released[slot]])] += 1
        self.released[slot] = first

    def slots(self, seqs) -> list:
        """The slots of `seqs`; raises for an unknown, freed or repeated one."""
        out = [self.slot(s) for s in seqs]
        if len(set(out)) != len(out):
            raise ValueError(f"PagedKVCache: a sequence is named twice in {list(seqs)}")
        return out

    @staticmethod
    def _counts(n, slots) -> list:
        """One count per slot from `n`: an int (>= 1, the same for all) or one count (>= 0) per sequence."""
        if isinstance(n, int):
            if n < 1:
                raise ValueError(f"PagedKVCache.append: {n} new keys")
            return [n] * len(slots)
        counts = [int(c) for c in n]
        if len(counts) != len(slots) or any(c < 0 for c in counts):
            raise ValueError(f"PagedKVCache.append: counts {counts} for {len(slots)} sequences - one count >= 0 per sequence")
        return counts

    def reserve(self, seqs, n):
        """Pages for n more keys of every sequence of `seqs` - n an int, or one count per sequence (0: the sequence takes no page) -
        taken before anything is launched: (slots, lengths before, pages taken per slot).  Raises with no page taken and nothing
        changed; the lengths advance with commit(), and rollback() hands the pages back when the launch is refused after all."""
        slots = self.slots(seqs)
        need = []
        for seq, s, c in zip(seqs, slots, self._counts(n, slots)):
            pages = (self.lengths[s] + c + PAGE_KEYS - 1) // PAGE_KEYS
            if c and pages > self.max_pages_per_seq:
                raise RuntimeError(f"PagedKVCache.append: sequence {seq} would hold {self.lengths[s] + c} keys = {pages} pages, beyond "
                                   f"max_pages_per_seq = {self.max_pages_per_seq}")
            need.append(pages - self.pages_of[s] if c else 0)
        if sum(need) > len(self._free_pages):
            raise RuntimeError(f"PagedKVCache.append: out of pages - {sum(need)} needed, {len(self._free_pages)} of {self.num_pages} free")
        for s, k in zip(slots, need):
            for _ in range(k):
                self.table[s][self.pages_of[s]] = page = self._free_pages.pop()
                self._owners[page] = 1
                self.pages_of[s] += 1
        return slots, [self.lengths[s] for s in slots], need

    def rollback(self, slots, taken) -> None:
        """Undo a reserve() whose launch did not happen: the pages go back in the order that makes the next reserve() take the same."""
        for s, k in zip(reversed(slots), reversed(taken)):
            for _ in range(k):
                self.pages_of[s] -= 1
                self._owners[self.table[s][self.pages_of[s]]] = 0
                self._free_pages.append(self.table[s][self.pages_of[s]])

    def commit(self, slots, n) -> None:
        """The lengths after the launch: n as in reserve()."""
        for s, c in zip(slots, self._counts(n, slots)):
            self.lengths[s] += c

    def fork(self, parents):
        """One new sequence per entry of `parents` (repeats allowed), each of its parent's length: (children, parents' slots,
        children's slots, lengths).  A child's row takes the parent's full pages, their counts raised, and - where the length is no
        multiple of 16 - one fresh page for the open block, which the launch fills.  All or nothing: the slots and pages of the
        whole call are counted first; out of either raises RuntimeError with nothing taken.  rollback_fork() undoes it."""
        parents = list(parents)
        src = [self.slot(p) for p in parents]
        lens = [self.lengths[s] for s in src]
        pages = sum(1 for n in lens if n % PAGE_KEYS)
        if len(parents) > len(self._free_slots):
            raise RuntimeError(f"PagedKVCache.fork: {len(parents)} new sequences, {len(self._free_slots)} of {self.max_seqs} sequence slots free")
        if pages > len(self._free_pages):
            raise RuntimeError(f"PagedKVCache.fork: out of pages - {pages} needed, {len(self._free_pages)} of {self.num_pages} free")
        children, dst, shared = [], [], {}
        for s, n in zip(src, lens):
            child = self.alloc()
            d, full = self._slot[child], n // PAGE_KEYS
            row, gone = self.table[d], self.released[s]
            if full:
                row[:full] = self.table[s][:full]  # (the stale entries too: valid indices, read by nothing)
                if s not in shared:
                    shared[s] = np.array(row[gone:full], dtype=np.int64)
                self._owners[shared[s]] += 1       # the live entries only: a released page is not the parent's to share
            if n % PAGE_KEYS:
                row[full] = page = self._free_pages.pop()
                self._owners[page] = 1
            self.pages_of[d], self.lengths[d], self.released[d] = (n + PAGE_KEYS - 1) // PAGE_KEYS, n, gone
            children.append(child), dst.append(d)
        return children, src, dst, lens

    def rollback_fork(self, children) -> None:
        """Undo a fork() whose launch did not happen: the ids, slots and pages go back so that the next call takes the same."""
        for child in reversed(children):
            self.free(child)
        self._next_seq -= len(children)

    def export(self, seqs) -> dict:
        """The books of `seqs` as plain host data, for another table to adopt: {"pages": the distinct pages the sequences hold (their
        row entries released .. pages_of - 1), in order of first appearance - a page two of them hold appears once; "seqs": per
        sequence (length, released, local row)}, a local row being the sequence's row with every held entry replaced by the page's
        position in "pages" and the released entries by 0.  Nothing in the books changes."""
        local, out = {}, []
        for s in self.slots(seqs):
            gone = self.released[s]
            row = [0] * gone + [local.setdefault(p, len(local)) for p in self.table[s][gone:self.pages_of[s]]]
            out.append((self.lengths[s], gone, row))
        return {"pages": list(local), "seqs": out}

    def adopt(self, books):
        """New sequences with the books export() gave (of this table or another): (seqs, slots, page map - the page of this table that
        stands for each entry of books["pages"]).  All or nothing, as fork: the slots of all sequences, the free pages of all
        distinct pages and max_pages_per_seq for every row are counted first; short of any raises RuntimeError with nothing taken.
        Rows stay indexed by absolute key / 16: released entries become 0 - a valid index that nothing reads -, `released` and
        `lengths` are the exported ones, and a page has as many owners as adopted sequences name it.  rollback_adopt() undoes it."""
        n, seqs = len(books["pages"]), list(books["seqs"])
        named = set()
        for length, gone, row in seqs:
            if length < 0 or len(row) != (length + PAGE_KEYS - 1) // PAGE_KEYS or not 0 <= gone <= length // PAGE_KEYS:
                raise ValueError(f"PagedKVCache.adopt: a sequence of {length} keys with a row of {len(row)} entries, {gone} released")
            named.update(row[gone:])
        if named != set(range(n)):
            raise ValueError(f"PagedKVCache.adopt: the rows name pages {sorted(named)} of {n}")
        if len(seqs) > len(self._free_slots):
            raise RuntimeError(f"PagedKVCache.adopt: {len(seqs)} new sequences, {len(self._free_slots)} of {self.max_seqs} sequence slots free")
        if n > len(self._free_pages):
            raise RuntimeError(f"PagedKVCache.adopt: out of pages - {n} needed, {len(self._free_pages)} of {self.num_pages} free")
        for length, _, row in seqs:
            if len(row) > self.max_pages_per_seq:
                raise RuntimeError(f"PagedKVCache.adopt: a sequence of {length} keys = {len(row)} pages, beyond max_pages_per_seq = "
                                   f"{self.max_pages_per_seq}")
        pages = [self._free_pages.pop() for _ in range(n)]
        out, slots = [], []
        for length, gone, row in seqs:
            seq = self.alloc()
            s = self._slot[seq]
            mine = [pages[i] for i in row[gone:]]
            self.table[s][:len(row)] = [0] * gone + mine
            if mine:
                self._owners[np.array(mine)] += 1
            self.pages_of[s], self.lengths[s], self.released[s] = len(row), length, gone
            out.append(seq), slots.append(s)
        return out, slots, pages

    def rollback_adopt(self, seqs) -> None:
        """Undo an adopt() whose launch did not happen: the ids, slots and pages go back so that the next call takes the same."""
        held = lambda s: self.table[s][self.released[s]:self.pages_of[s]]
        pages = list(dict.fromkeys(p for seq in seqs for p in held(self.slot(seq))))  # in the order adopt() took them
        if pages:
            self._owners[np.array(pages)] = 0
        self._free_pages.extend(reversed(pages))
        for seq in reversed(seqs):
            s = self._slot.pop(seq)
            self.pages_of[s] = self.lengths[s] = self.released[s] = 0
            self._free_slots.append(s)
        self._next_seq -= len(seqs)

    def prefix_groups(self, slots, lens, chunk_of) -> list:
        """The sequences of one call - in `slots`, of `lens` keys - grouped by the prefix they hold on the SAME pages: a list of
        (members, shared_keys), members the call indices in ascending order (the first is the group's leader), the groups ordered by
        their first member, every call index in exactly one group.  chunk_of(length): the decode kernels' chunk length.
        A sequence is eligible with no released page and at least one full page (16 keys).  Eligible sequences cluster by
        (chunk_of(len), first page); of a cluster of two or more, n = the leading row entries equal in ALL members' rows, capped at
        min(len) // 16 - an open block is never shared -, and P = 16 n keys.  P below the chunk length shares no chunk: the cluster
        then dissolves into groups of one, as everything not eligible is (P = 0).  ONE level: a subset that shares more than its
        whole cluster does (a beam tree) still gets the cluster's P."""
        clusters = {}
        for i, (s, t) in enumerate(zip(slots, lens)):
            if self.released[s] == 0 and t >= PAGE_KEYS:
                clusters.setdefault((chunk_of(t), self.table[s][0]), []).append(i)
        shared = {}  # leader -> (members, P)
        for (chunk, _), mem in clusters.items():
            if len(mem) < 2:
                continue
            first, n = self.table[slots[mem[0]]], min(lens[i] for i in mem) // PAGE_KEYS
            for i in mem[1:]:  # (whole-slice compares: beams that share everything below their open blocks cost one each)
                row = self.table[slots[i]]
                if row[:n] != first[:n]:
                    n = next(e for e, (x, y) in enumerate(zip(row, first)) if x != y)
            if PAGE_KEYS * n >= chunk:
                shared[mem[0]] = (mem, PAGE_KEYS * n)
        grouped = {i for mem, _ in shared.values() for i in mem[1:]}
        return [shared.get(i, ([i], 0)) for i in range(len(slots)) if i not in grouped]

    def snapshot(self, seqs=()):
        """The books, and the table rows of `seqs` - what restore() needs to put back sequences that were freed since."""
        return (self._free_pages[:], self._free_slots[:], dict(self._slot), self._next_seq, self.pages_of[:], self.lengths[:], self._owners.copy(),
                self.released[:], {self.slot(s): self.table[self.slot(s)][:] for s in seqs})

    def restore(self, snap) -> None:
        self._free_pages, self._free_slots, self._slot, self._next_seq, self.pages_of, self.lengths, self._owners = (
            snap[0][:], snap[1][:], dict(snap[2]), snap[3], snap[4][:], snap[5][:], snap[6].copy())
        self.released = snap[7][:]
        for s, row in snap[-1].items():
            self.table[s][:] = row


class PagedKVCache:
    """K and V of one attention layer for MANY sequences of their own lengths, as QuantizedKVCache's codes and exponents in pages of 16
    keys (include/lqer_hip.h "paged KV pool"): memory is paid per page in use, a freed sequence's pages serve the next, nothing is copied
    to grow.  A batch of a decode step addresses any subset of the live sequences in any order - continuous batching.

    .alloc() -> seq    a new, empty sequence;  .free(seq)  its pages and slot back to the pool (no clearing: pages are reused dirty)
    .append(seqs, k, v)   k / v [len(seqs), kv_heads, n, head_dim]: n more keys for every sequence of `seqs`.  The pages of the WHOLE
                       call are taken before anything is launched; out of pages, beyond max_pages_per_seq, an unknown, freed or
                       repeated seq raise with the pool untouched and no page taken - and so does a refusal of the library itself:
                       the reservation is rolled back
    .append_ragged(seqs, k, v, counts)   k / v [sum(counts), kv_heads, head_dim]: counts[b] more keys for seqs[b] - the decoders' one
                       key and the arrivals' prompt chunks of a scheduler step in ONE launch, with append's bytes, books and refusals
    .length(seq);  .pages_free;  .nbytes
    .to_dense(seq) -> QuantizedKVCache (batch 1) with the sequence's bytes - an export, and the test hook (more than 8 query rows
                       need no copy: attention_flexible_paged(kernel="prefill"));  .dequantized(seq) -> (K, V) [1, kv_heads, length,
                       head_dim] fp32, for tests
    .fork(seq, n=1) / .fork_many(parents) -> new sequences that hold their parent's keys: a page is one K quantizer block, an append
                       rewrites only the block at length / 16 and those after it, so a FULL page is never written again and is
                       shared by reference - no copy-on-write; a child costs one page (the open block, if there is one) and one
                       launch for the whole set
    .reorder(seqs, parent_idx) -> the beam step: the ids of the beams that continue seqs[parent_idx[i]]
    .pages_shared      pages with more than one owner

    Taking speculated tokens back: `snap, = cache.fork(seq)`, append the speculated block to `seq` and attend; if only the first m of
    its keys are accepted, `cache.free(seq)` and append those m keys' k / v - the step still has them - to `snap`, which goes on as
    the sequence: the bits of one that only ever saw the m.  There is no in-place crop: the raw keys of a closed block are gone,
    so a shortened block cannot be given the codes and exponents it would have had.
    The recipe is a draft TREE's too (attention_flexible_paged_tree): fork a snapshot, append_ragged the WHOLE tree - its nodes in an
    order that puts parents before children -, attend with the nodes' parents, free the sequence and append the rows of k / v of the
    accepted root-to-leaf path to the snapshot.

    window=W (None: keep everything): a SLIDING-WINDOW cache - attention_flexible_paged then defaults to the window rule (a query at
    position p sees keys p - W < j <= p), and `append` hands back the pages nothing can see any more: for each addressed sequence
    those wholly below min(T_after - W - 7, 16 (T_before // 16)) - a later call of up to 8 query rows starts at key T - 8 - W + 1
    >= T_after - W - 7, and the append itself touches the block at T_before // 16 and those after it.  The release comes BEFORE the
    reservation, so the append can take the pages it has just freed and a pool sized for the window keeps running however long the
    sequences grow; it is undone, with the books as they were, when the reservation or the launch is refused.  After an append of
    n <= W + 7 keys a sequence holds at most (W + 37) // 16 pages (.pages_held(seq)).  Forks share pages as ever: a released page
    goes back to the pool with its last owner.  The table's rows stay indexed by absolute key / 16 (no ring), so max_pages_per_seq
    still bounds a sequence's total length.  The early keys of a sequence that has released pages are gone: to_dense() and
    dequantized() raise ValueError for it.

    max_query_rows=R (None: 8, and everything above as it stands; else an int >= 8): the most query rows per sequence a later
    attention call may bring.  It switches on the prefill kernel's window rule - attention_flexible_paged(kernel="prefill" / "auto")
    and the prefill call of attention_flexible_paged_ragged beyond the window (lqer_attention_q_paged_window,
    lqer_attention_q_paged_ragged_window): a long prompt in chunks, a second turn, a prompt chunk beside windowed decoders - and it
    widens what `append` keeps: a sequence gives up the pages wholly below min(T_after - W - (R - 1), 16 (T_before // 16)); R = 8 is
    the rule above, term for term.  Two facts, for appends of at most W + R - 1 keys each:
      - after such an append a sequence holds at most (W + R + 29) // 16 pages, and the bound is reached (R = 8: (W + 37) // 16);
      - for every later call of s <= R rows on a sequence of T keys, 16 released <= max(0, T - s - W + 1): the page of the first key
        the call's first row sees is still there.  A call that breaks it (more rows than R) raises ValueError: the keys are gone.
    With window=None nothing is ever released, and R only allows an explicit window= on the prefill route.

    code_bits (None or 8: a byte per code, the pool as ever; 4; or a pair (k_bits, v_bits)): 4 stores the operand's codes as NIBBLES -
    for configs of width <= 4 (ValueError otherwise, before anything is allocated), where sign and magnitude are exactly four bits:
    2 d (1/2 + 1/16) bytes per token and kv head instead of 2 d (1 + 1/16), 144 B against 272 B at d = 128, so the same memory holds
    1.89x the tokens.  The values are those of the byte pool of the same configs - the storage changes no rounding - and every method
    and every attention_flexible_paged* function works unchanged: `.nbytes` is the smaller pool (lqer_kv_pool_bytes_fmt), to_dense()
    gives a byte QuantizedKVCache (lqer_kv_pool_gather_fmt widens the nibbles), fork copies the smaller item.  K and V choose on
    their own: (8, 4) keeps a wide K beside a 4-bit V.  shared_prefix=True runs the ungrouped call on such a pool (the grouped
    kernels are not instantiated for nibble codes; the bits are the same by that feature's contract).

    Sequences out of the pool and into one (lqer_kv_pool_copy: a list of pages and a list of slots' staging rows from one pool to
    another in one launch, bytes as they are): .export(seqs, device=None) -> KVPoolImage, a small pool in the library's own layout
    with its books, on the device or ("cpu") in pinned host memory, the sequences still live; .adopt(image) -> new sequences;
    .swap_out(seqs) = export to the host + free (preemption: when append raises "out of pages" a victim's bytes leave and come back
    instead of being recomputed), .swap_in(image) = adopt; .adopt_from(other, seqs): pool to pool with no image (a prefill pool to a
    decode pool; `other` may be this cache).  An image survives state_dict() / torch.save / torch.load / from_state_dict().  THE
    GUARANTEE: an adopted sequence is from then on a sequence like any other - every attention_flexible_paged* function gives the
    SAME BITS on it as on the sequence it was exported from, and so does every later append / append_ragged (the staging rows
    travelled), fork and to_dense - whatever pages it lands on, whichever pool it lands in, whether or not the image went through
    the host or a file.  Nibble pools, sequences with released pages (adopted only under the same window and max_query_rows:
    ValueError otherwise) and forks - a shared page travels once and is shared again - need no special case."""

    covers = staticmethod(QuantizedKVCache.covers)

    def __init__(self, num_pages: int, max_seqs: int, kv_heads: int, head_dim: int, cfg0: dict, cfg1: dict, dtype: torch.dtype, device,
                 max_pages_per_seq=None, window=None, max_query_rows=None, code_bits=None):
        _check_covers("PagedKVCache", cfg0, cfg1, head_dim, dtype)
        self.code_bits = _code_bits(code_bits, _attn_fmts(cfg0, cfg1))  # (raises before anything is allocated)
        _window_arg("PagedKVCache", window, None, causal=True)  # (no call, so no causal to ask for)
        if max_query_rows is not None and (not isinstance(max_query_rows, int) or isinstance(max_query_rows, bool)
                                           or max_query_rows < _ATTN_DECODE_MAX_S):
            raise ValueError(f"PagedKVCache: max_query_rows {max_query_rows!r} - None or a number of query rows >= {_ATTN_DECODE_MAX_S}")
        self.window, self.max_query_rows = window, max_query_rows
        self.pt = PageTable(num_pages, max_seqs, max_pages_per_seq)
        if kv_heads < 1 or kv_heads > _MAX_GRID_Z or max_seqs > _MAX_GRID_Z or self.pt.max_len > 1 << 30:
            raise ValueError(f"PagedKVCache: kv_heads {kv_heads}, max_seqs {max_seqs}, max_pages_per_seq {self.pt.max_pages_per_seq}")
        self.kv_heads, self.head_dim, self.dtype, self.device = kv_heads, head_dim, dtype, torch.device(device)
        self.cfg0, self.cfg1 = cfg0, cfg1
        self.fmts = _attn_fmts(cfg0, cfg1)  # Q, K^T, P, V
        self.nibble = 4 in self.code_bits  # some code section holds nibbles: K and V then carry the kind that says which, in every call
        if self.nibble:
            for i, bits in zip((1, 3), self.code_bits):
                if bits == 4:
                    self.fmts[i] = ops.nibble_qfmt(self.fmts[i])
        self.buf = torch.empty(pool_bytes(dtype, num_pages, max_seqs, kv_heads, head_dim, *self._code_fmts()),
                               dtype=torch.uint8, device=self.device)
        # the device copies of the metadata: the table (rows updated when they change), the slots and the lengths of the current call
        self.table = torch.zeros(max_seqs, self.pt.max_pages_per_seq, dtype=torch.int32, device=self.device)
        self._slots = torch.zeros(max_seqs, dtype=torch.int32, device=self.device)
        self._lens = torch.zeros(max_seqs, dtype=torch.int32, device=self.device)
        self._starts = torch.zeros(max_seqs + 1, dtype=torch.int32, device=self.device)  # per-sequence counts of a call, as token starts
        self._groups = torch.zeros(4 * max_seqs + 1, dtype=torch.int32, device=self.device)  # the prefix groups of a call (_call_groups)

    num_pages = property(lambda self: self.pt.num_pages)
    max_seqs = property(lambda self: self.pt.max_seqs)
    pages_free = property(lambda self: self.pt.pages_free)
    nbytes = property(lambda self: self.buf.numel())

    def alloc(self) -> int:
        return self.pt.alloc()

    def free(self, seq: int) -> None:
        self.pt.free(seq)

    def length(self, seq: int) -> int:
        return self.pt.length(seq)

    def pages_held(self, seq: int) -> int:
        return self.pt.pages_held(seq)

    def _pool_args(self):
        return (self.buf.data_ptr(), self.buf.numel(), self.pt.num_pages, self.pt.max_seqs, self.table.data_ptr(), self.pt.max_pages_per_seq)

    def _call_meta(self, slots, lens, max_len=None):
        """seq_slots and lens of one call on the device: ordinary copies on the current stream, ordered before the launches.
        max_len: the bound handed to the library - the table's room, or a tighter one that still covers `lens`."""
        n = len(slots)
        self._slots[:n].copy_(torch.tensor(slots, dtype=torch.int32))
        self._lens[:n].copy_(torch.tensor(lens, dtype=torch.int32))
        return self._slots.data_ptr(), self._lens.data_ptr(), self.pt.max_len if max_len is None else max_len

    @torch.no_grad()
    def append(self, seqs, k: torch.Tensor, v: torch.Tensor) -> None:
        seqs = list(seqs)
        want = (len(seqs), self.kv_heads, self.head_dim)
        if k.dim() != 4 or (k.shape[0], k.shape[1], k.shape[3]) != want or k.shape != v.shape or k.dtype != self.dtype or v.dtype != self.dtype:
            raise ValueError(f"PagedKVCache.append: k {tuple(k.shape)} {k.dtype} / v {tuple(v.shape)} {v.dtype} for {len(seqs)} sequences of "
                             f"[{self.kv_heads}, n, {self.head_dim}] {self.dtype}")
        if k.device != self.buf.device or v.device != self.buf.device:
            raise ValueError(f"PagedKVCache.append: k on {k.device} / v on {v.device} for a pool on {self.buf.device}")
        n = k.shape[2]
        if n == 0 or not seqs:
            self.pt.slots(seqs)
            return
        self._append(seqs, n, self._launch_append, k, v)

    def _append(self, seqs, n, launch, k, v) -> None:
        """The body of both appends, n an int or one count per sequence: release what the window lets go, reserve the pages of the
        whole call, launch(slots, lengths before, pages taken per slot, k, v, n) - the caller's _launch_* as the instance has it now -,
        commit the lengths - and, when the reservation or the launch is refused, the books as they were."""
        undo = self._release_outside_window(seqs, n) if self.window is not None else []
        try:
            slots, lens, taken = self.pt.reserve(seqs, n)  # (raises with nothing taken)
            try:
                launch(slots, lens, taken, k, v, n)
            except BaseException:
                self.pt.rollback(slots, taken)  # (the device rows of the table may keep the entries: nothing reads beyond a length)
                raise
        except BaseException:
            for u in reversed(undo):
                self.pt.unrelease(*u)
            raise
        self.pt.commit(slots, n)

    def _release_outside_window(self, seqs, n) -> list:
        """Before an append of n keys to `seqs` - an int, or one count per sequence, each sequence then by its own; a count of 0 leaves
        the sequence alone - (validated here, so a bad call releases nothing): every sequence gives up the pages no later call can
        see and this append does not touch.  Returns what PageTable.unrelease needs, in the order of the calls."""
        undo = []
        slots = self.pt.slots(seqs)
        for seq, s, c in zip(seqs, slots, self.pt._counts(n, slots)):
            if not c:
                continue
            t = self.pt.lengths[s]
            first = self.pt.released[s]
            rows = _ATTN_DECODE_MAX_S if self.max_query_rows is None else self.max_query_rows  # a later call's most query rows
            freed = self.pt.release(seq, min(t + c - self.window - (rows - 1), PAGE_KEYS * (t // PAGE_KEYS)))
            if self.pt.released[s] != first:
                undo.append((seq, first, freed))
        return undo

    def _upload_rows(self, slots, taken) -> None:
        """The table rows that took pages, to the device."""
        for s, t in zip(slots, taken):
            if t:
                self.table[s].copy_(torch.tensor(self.pt.table[s], dtype=torch.int32))

    def _launch_append(self, slots, lens, taken, k, v, n) -> None:
        self._upload_rows(slots, taken)
        if k.stride(3) != 1:
            k = k.contiguous()
        if v.stride(3) != 1:
            v = v.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lqer_kv_pool_append(*self._pool_args(), *self._call_meta(slots, lens), k.data_ptr(), v.data_ptr(), _tri(k), _tri(v),
                                                      ops._DT[self.dtype], len(slots), self.kv_heads, self.head_dim, n, C.byref(self.fmts[1]),
                                                      C.byref(self.fmts[3]), ops._stream(self.device)),
                       "lqer_kv_pool_append")

    @torch.no_grad()
    def append_ragged(self, seqs, k: torch.Tensor, v: torch.Tensor, counts) -> None:
        """append() with a count of its own per sequence - a scheduler step in which most sequences take one key and a few a prompt
        chunk - in ONE launch (lqer_kv_pool_append_ragged): k / v [sum(counts), kv_heads, head_dim], sequence seqs[b] taking rows
        sum(counts[:b]) .. + counts[b] - 1; a count of 0 leaves its sequence alone.  The pool's bytes afterwards are those of one
        append() per sequence.  Reservation, refusals, rollback and - on a window=W cache - the release of unseen pages, each
        sequence by its own count, are append()'s: a refused call leaves the books and the pool as they were."""
        seqs, counts = _ragged_counts("PagedKVCache.append_ragged", seqs, counts)
        want = (sum(counts), self.kv_heads, self.head_dim)
        if k.dim() != 3 or tuple(k.shape) != want or k.shape != v.shape or k.dtype != self.dtype or v.dtype != self.dtype:
            raise ValueError(f"PagedKVCache.append_ragged: k {tuple(k.shape)} {k.dtype} / v {tuple(v.shape)} {v.dtype} for counts {counts} of "
                             f"[sum(counts), {self.kv_heads}, {self.head_dim}] {self.dtype}")
        if k.device != self.buf.device or v.device != self.buf.device:
            raise ValueError(f"PagedKVCache.append_ragged: k on {k.device} / v on {v.device} for a pool on {self.buf.device}")
        if not any(counts):
            self.pt.slots(seqs)
            return
        self._append(seqs, counts, self._launch_append_ragged, k, v)

    def _call_starts(self, counts):
        """The token starts [len(counts) + 1] of a call with per-sequence counts on the device: one copy, as _call_meta's."""
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        self._starts[:len(starts)].copy_(torch.tensor(starts, dtype=torch.int32))
        return self._starts.data_ptr()

    def _call_groups(self, groups):
        """The prefix groups of a call (PageTable.prefix_groups) on the device, in ONE copy as _call_meta's: grp_of [n], grp_starts
        [groups + 1], grp_members [n] and grp_keys [groups] one behind the other - their four pointers and the group count."""
        n = sum(len(mem) for mem, _ in groups)
        of, starts, members = [0] * n, [0], []
        for i, (mem, _) in enumerate(groups):
            for b in mem:
                of[b] = i
            members += mem
            starts.append(len(members))
        flat = of + starts + members + [p for _, p in groups]
        self._groups[:len(flat)].copy_(torch.tensor(flat, dtype=torch.int32))
        at = (0, n, n + len(starts), 2 * n + len(starts))
        return tuple(self._groups.data_ptr() + 4 * x for x in at) + (len(groups),)

    def _launch_append_ragged(self, slots, lens, taken, k, v, counts) -> None:
        self._upload_rows(slots, taken)
        if k.stride(2) != 1:
            k = k.contiguous()
        if v.stride(2) != 1:
            v = v.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().lqer_kv_pool_append_ragged(*self._pool_args(), *self._call_meta(slots, lens), self._call_starts(counts), max(counts),
                                                             k.data_ptr(), v.data_ptr(), _pair(k), _pair(v), ops._DT[self.dtype], len(slots),
                                                             self.kv_heads, self.head_dim, sum(counts), C.byref(self.fmts[1]),
                                                             C.byref(self.fmts[3]), ops._stream(self.device)),
                       "lqer_kv_pool_append_ragged")

    # ---- sequences over shared pages (lqer_kv_pool_fork) ----
    def fork(self, seq: int, n: int = 1) -> list:
        """n new sequences that hold seq's keys: fork_many([seq] * n)."""
        if n < 1:
            raise ValueError(f"PagedKVCache.fork: {n} children")
        return self.fork_many([seq] * n)

    @torch.no_grad()
    def fork_many(self, parents) -> list:
        """One new sequence per entry of `parents` (repeats allowed) with its parent's keys - samples of one prompt, sequences behind
        one system prompt, beams - from then on a sequence like any other: it appends and attends with the bits of a sequence that was
        appended the same keys itself, and is freed on its own.  The parent's full pages are shared by reference; what one launch for
        the whole set copies is the open block (a page of the child's own) and the staging rows per child.  Slots and pages of the
        whole call are taken first; out of either, an unknown or freed parent, or a refusal of the library raise with the pool and
        the books as they were.  A parent of length 0 gives empty children, and nothing is launched."""
        parents = list(parents)
        if not parents:
            return []
        children, src, dst, lens = self.pt.fork(parents)  # (raises with nothing taken)
        try:
            self._launch_fork(src, dst, lens)
        except BaseException:
            self.pt.rollback_fork(children)  # (the device rows of the table may keep the entries: nothing reads beyond a length)
            raise
        return children

    def _with_code_fmts(self, entry):
        """A pool entry that takes no formats (gather, fork) as this pool calls it: `entry` and no formats on a pool of byte codes, its
        _fmt sibling and the K and V formats, which name the storage, on one with nibble codes."""
        return (entry + "_fmt", (C.byref(self.fmts[1]), C.byref(self.fmts[3]))) if self.nibble else (entry, ())

    def _launch_fork(self, src, dst, lens) -> None:
        """The children's table rows, then the one launch.  Everything the device needs goes up in ONE small copy - the three arrays of
        the call, and (child's slot, entry, page) of every open block - and the rows are made on the device: the parent's row, which
        names the shared pages, with the child's own page put in at the open block (entries beyond a length are read by nothing)."""
        pairs = [(s, d, n) for s, d, n in zip(src, dst, lens) if n]
        if not pairs:
            return
        src, dst, lens = (list(x) for x in zip(*pairs))
        n = len(pairs)
        own = [(d, t // PAGE_KEYS, self.pt.table[d][t // PAGE_KEYS]) for d, t in zip(dst, lens) if t % PAGE_KEYS]
        pad = [0] * (n - len(own))
        meta = torch.tensor([src, dst, lens] + [[x[i] for x in own] + pad for i in range(3)], dtype=torch.int32).to(self.device)
        idx = meta.long()
        self.table.index_copy_(0, idx[1], self.table.index_select(0, idx[0]))
        if own:
            k = len(own)
            self.table.index_put_((idx[3, :k], idx[4, :k]), meta[5, :k])
        with torch.cuda.device(self.device):
            name, fmts = self._with_code_fmts("lqer_kv_pool_fork")
            _lib.check(getattr(_lib.lib(), name)(self.buf.data_ptr(), self.buf.numel(), ops._DT[self.dtype], self.pt.num_pages, self.pt.max_seqs,
                                                 self.kv_heads, self.head_dim, self.table.data_ptr(), self.pt.max_pages_per_seq,
                                                 meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), n, *fmts, ops._stream(self.device)),
                       name)

    @torch.no_grad()
    def reorder(self, seqs, parent_idx) -> list:
        """The beam step: the ids of the new beams, beam i continuing seqs[parent_idx[i]].  The first beam that continues a parent
        keeps the parent's id and nothing is copied; further ones are forks (one launch for all of them); parents nobody continues
        are freed - before pages are taken, so their pages can serve the forks.  A pure permutation launches nothing and takes no
        page.  A call the pool cannot serve raises RuntimeError with the pool and the books as they were, and so does one the library
        refuses."""
        seqs, parent_idx = list(seqs), [int(j) for j in parent_idx]
        self.pt.slots(seqs)
        if any(not 0 <= j < len(seqs) for j in parent_idx):
            raise ValueError(f"PagedKVCache.reorder: parent_idx {parent_idx} for {len(seqs)} sequences")
        out, forks, kept = [], [], set()
        for j in parent_idx:
            out.append(None if j in kept else seqs[j])
            if j in kept:
                forks.append(seqs[j])
            kept.add(j)
        dropped = [s for j, s in enumerate(seqs) if j not in kept]
        if not forks and not dropped:
            return out
        snap = self.pt.snapshot(dropped)
        try:
            for s in dropped:
                self.pt.free(s)
            children = iter(self.fork_many(forks))  # (out of slots or pages: raises with nothing taken)
        except BaseException:
            self.pt.restore(snap)
            for s, row in snap[-1].items():  # the freed sequences' device rows, which a child may have taken
                self.table[s].copy_(torch.tensor(row, dtype=torch.int32))
            raise
        return [next(children) if s is None else s for s in out]

    # ---- sequences out of the pool and into one (lqer_kv_pool_copy) ----
    def _code_fmts(self) -> tuple:
        """The K and V formats where they name the storage (a pool with nibble codes), nothing on a pool of byte codes."""
        return (self.fmts[1], self.fmts[3]) if self.nibble else ()

    def _signature(self) -> tuple:
        """What two pools must agree on for bytes to move between them - dtype, kv_heads, head_dim, the K and V format fields (their
        kinds name the storage), code_bits - and, last, what decides which pages a sequence may have released: window (0: none) and
        the query rows a later call may bring."""
        fields = lambda f: (f.kind, f.width, f.block, f.exp_width, f.exp_bias)
        rows = _ATTN_DECODE_MAX_S if self.max_query_rows is None else self.max_query_rows
        return (ops._DT[self.dtype], self.kv_heads, self.head_dim, *fields(self.fmts[1]), *fields(self.fmts[3]), *self.code_bits,
                self.window or 0, rows)

    def _check_signature(self, who: str, signature, books) -> None:
        mine, theirs = self._signature(), tuple(signature)
        if len(theirs) != len(mine) or theirs[:-2] != mine[:-2]:
            raise ValueError(f"{who}: sequences of a pool with (dtype, kv_heads, head_dim, K format, V format, code_bits) = {theirs[:-2]} for one "
                             f"with {mine[:-2]} - bytes move as they are, between pools of one geometry, formats and storage")
        if theirs[-2:] != mine[-2:] and any(gone for _, gone, _ in books["seqs"]):
            raise ValueError(f"{who}: a sequence has released pages under (window, max_query_rows) = {theirs[-2:]}, this cache has {mine[-2:]} - "
                             "the keys below are gone, and only that window rule never reads them")

    @torch.no_grad()
    def export(self, seqs, device=None) -> KVPoolImage:
        """The sequences' bytes as a KVPoolImage, on this cache's device or (device="cpu") in pinned host memory; the sequences stay
        live.  The id lists go up in one small copy, ONE lqer_kv_pool_copy writes a device image - the distinct pages, a page shared
        by forks once, and a slot per sequence - and for the host one non-blocking copy follows on the current stream; image.ready is
        recorded behind it.  Unknown, freed or repeated sequences raise, as elsewhere; so does an empty list."""
        seqs = list(seqs)
        host = device is not None and torch.device(device).type == "cpu"
        if not seqs or (device is not None and not host and torch.empty(0, device=device).device != self.buf.device):
            raise ValueError(f"PagedKVCache.export: {len(seqs)} sequences to {device!r} - at least one, to 'cpu' or the pool's device {self.buf.device}")
        books, slots = self.pt.export(seqs), self.pt.slots(seqs)
        n, m = len(books["pages"]), len(seqs)
        pages = max(n, 1)  # (the library sizes no pool of 0 pages)
        img = torch.empty(pool_bytes(self.dtype, pages, m, self.kv_heads, self.head_dim, *self._code_fmts()), dtype=torch.uint8, device=self.buf.device)
        ids = torch.tensor(books["pages"] + list(range(n)) + slots + list(range(m)), dtype=torch.int32).to(self.buf.device)
        pool_copy(self.buf, self.pt.num_pages, self.pt.max_seqs, img, pages, m, self.dtype, self.kv_heads, self.head_dim, ids, n, m, *self._code_fmts())
        if host:
            dev_img, img = img, torch.empty(img.numel(), dtype=torch.uint8, pin_memory=True)
            with torch.cuda.device(self.buf.device):
                img.copy_(dev_img, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.buf.device))
        return KVPoolImage(img, pages, {"pages": list(range(n)), "seqs": books["seqs"]}, self._signature(), ready)

    def _adopt(self, who: str, signature, books, source) -> list:
        """The body of adopt and adopt_from: the checks, the reservation (PageTable.adopt: all or nothing), source() -> (buffer on this
        device, its pages, its slots, page ids, slot ids), the new rows and the id lists up in one copy each, ONE lqer_kv_pool_copy -
        and, when anything after the reservation is refused, the books as they were."""
        self._check_signature(who, signature, books)
        seqs, slots, pages = self.pt.adopt(books)  # (raises with nothing taken)
        try:
            buf, src_pages, src_slots, page_ids, slot_ids = source()
            n, m = len(pages), len(slots)
            ids = torch.tensor(list(page_ids) + pages + list(slot_ids) + slots, dtype=torch.int32).to(self.buf.device)
            rows = torch.tensor([self.pt.table[s] for s in slots], dtype=torch.int32).to(self.buf.device)
            self.table.index_copy_(0, ids[2 * n + m:].long(), rows)
            pool_copy(buf, src_pages, src_slots, self.buf, self.pt.num_pages, self.pt.max_seqs, self.dtype, self.kv_heads, self.head_dim, ids, n, m,
                      *self._code_fmts())
        except BaseException:
            self.pt.rollback_adopt(seqs)  # (the device rows of the table may keep the entries: nothing reads beyond a length)
            raise
        return seqs

    @torch.no_grad()
    def adopt(self, image: KVPoolImage) -> list:
        """New sequences with the bytes of an image's - from this cache or another of the same signature, straight from export(), from
        the host or from a file: from then on sequences like any other.  The current stream waits on image.ready, a host image comes up
        in one copy, ONE lqer_kv_pool_copy puts the pages and staging rows where the books (PageTable.adopt) found room.  ValueError for
        an image of another dtype, head count, head dim, format or code_bits, and for a sequence with released pages into a cache of
        another window or max_query_rows; RuntimeError out of slots, pages or beyond max_pages_per_seq; a refusal leaves the books
        and the pool as they were."""
        def source():  # (behind the signature check: the image's geometry is this pool's)
            want = pool_bytes(self.dtype, image.pages, image.slots, self.kv_heads, self.head_dim, *self._code_fmts())
            if image.buf.dtype != torch.uint8 or image.buf.numel() != want or len(image.books["pages"]) > image.pages:
                raise ValueError(f"PagedKVCache.adopt: an image of {image.buf.numel()} B {image.buf.dtype} for {image.pages} pages and {image.slots} "
                                 f"slots ({want} B)")
            if image.ready is not None:
                torch.cuda.current_stream(self.buf.device).wait_event(image.ready)
            with torch.cuda.device(self.buf.device):
                buf = image.buf.to(self.buf.device, non_blocking=True)
            return buf, image.pages, image.slots, range(len(image.books["pages"])), range(image.slots)

        return self._adopt("PagedKVCache.adopt", image.signature, image.books, source)

    @torch.no_grad()
    def adopt_from(self, other: "PagedKVCache", seqs) -> list:
        """adopt(other.export(seqs)) without the image: ONE lqer_kv_pool_copy straight from other's pool into this one - a prefill
        pool handing its sequences to a decode pool, or (other is this cache) copies on pages of their own.  The sequences stay live
        in `other`; adopt's checks and rollback."""
        seqs = list(seqs)
        if not isinstance(other, PagedKVCache) or other.buf.device != self.buf.device or not seqs:
            raise ValueError(f"PagedKVCache.adopt_from: {len(seqs)} sequences of {type(other).__name__} - at least one, of a PagedKVCache on {self.buf.device}")
        books, slots = other.pt.export(seqs), other.pt.slots(seqs)
        return self._adopt("PagedKVCache.adopt_from", other._signature(), books,
                           lambda: (other.buf, other.pt.num_pages, other.pt.max_seqs, books["pages"], slots))

    @torch.no_grad()
    def swap_out(self, seqs) -> KVPoolImage:
        """export(seqs, device="cpu"), then free() of every sequence: preemption.  The frees come after the launch on the same stream,
        so whoever takes the pages next overwrites them only behind the copy."""
        seqs = list(seqs)
        image = self.export(seqs, device="cpu")
        for s in seqs:
            self.pt.free(s)
        return image

    def swap_in(self, image: KVPoolImage) -> list:
        """adopt(image)."""
        return self.adopt(image)

    pages_shared = property(lambda self: self.pt.pages_shared)

    @torch.no_grad()
    def to_dense(self, seq: int) -> QuantizedKVCache:
        slot, t = self.pt.slot(seq), self.pt.length(seq)
        if self.pt.released[slot]:
            raise ValueError(f"PagedKVCache.to_dense: sequence {seq} has released its first {self.pt.released[slot]} pages (window {self.window}) - "
                             f"its keys below {PAGE_KEYS * self.pt.released[slot]} are gone")
        dense = QuantizedKVCache(1, self.kv_heads, self.head_dim, self.cfg0, self.cfg1, self.dtype, self.device, capacity=max(t, PAGE_KEYS))
        if t:
            with torch.cuda.device(self.device):
                name, fmts = self._with_code_fmts("lqer_kv_pool_gather")
                _lib.check(getattr(_lib.lib(), name)(self.buf.data_ptr(), self.buf.numel(), ops._DT[self.dtype], self.pt.num_pages,
                                                     self.pt.max_seqs, self.kv_heads, self.head_dim, self.table.data_ptr(),
                                                     self.pt.max_pages_per_seq, slot, t, dense.buf.data_ptr(), dense.buf.numel(),
                                                     dense.capacity, *fmts, ops._stream(self.device)),
                           name)
        dense.length = t
        return dense

    def dequantized(self, seq: int):
        return self.to_dense(seq).dequantized()


KERNEL_AUTO = "auto"


@torch.no_grad()
def attention_flexible_paged(q, cache: PagedKVCache, seqs, scaling, causal=False, out_layout="bhsd", return_stats=False, ws=None,
                             kernel=KERNEL_DECODE, window=None, shared_prefix=False):
    """attention_flexible(q[b:b+1], K_b, V_b, cache.cfg0, cache.cfg1, scaling, causal=causal, kernel=kernel) for every sequence
    seqs[b] of a PagedKVCache, bit for bit, in ONE call over sequences of different lengths.
    q [len(seqs), h, s, d]; `causal`: key j of sequence b visible to query i iff j <= i + (length_b - s).
    kernel="decode" (the default): s <= 8, lqer_attention_q_decode_paged reads the pool's codes.  kernel="prefill": any s >= 1 - a prompt,
    a second turn, a chunk of a long prompt on sequences that already hold keys - through lqer_attention_q_paged: the prefill kernel's
    two images are written from the pool through the block table (no dense copy) and the kernel takes every sequence's own length;
    the library's bound max_len is then the longest addressed length rounded up to 128 (capped at the table's room), so the image
    workspace follows the batch at hand.  kernel="auto": decode for s <= 8, prefill beyond.
    There is no mask tensor - the per-sequence lengths are what a padding mask stood for - and no other route: an empty sequence,
    causal with s > a length, s > 8 with kernel="decode", an unknown `kernel`, a wrong dtype, device or head count raise ValueError.
    `out_layout` and `return_stats` as attention_flexible; ws: a uint8 workspace or None (the stream's).
    window=W >= 1 (default: the cache's window, None on a cache without one; needs causal=True, ValueError otherwise): sliding-window
    attention - the query at position p sees keys p - W < j <= p, W keys including its own.  lqer_attention_q_decode_paged_window gives,
    per sequence, the bits of attention_flexible(..., attention_mask=M, kernel="decode") on the FULL raw K and V with M = 0 inside the
    window and torch.finfo(dtype).min outside, without reading a page wholly below the window - so it runs on sequences whose old pages
    the cache has released.  On such sequences an explicit W must not exceed the cache's (the keys are gone).  kernel="prefill" (and
    "auto" beyond 8 rows) with a window: while every addressed length is <= W the rule changes nothing, nothing can have been released
    and the unwindowed call runs.  Beyond, a cache made with max_query_rows runs lqer_attention_q_paged_window - the prefill kernel's
    window rule, the bits of attention_flexible(..., attention_mask=M, kernel="prefill") on the full raw K and V, no page below the
    window read; a sequence that has released the page of the first key this call's first row sees (16 released > max(0, T - s - W +
    1): more rows than the cache was made for) raises ValueError.  A cache without max_query_rows raises ValueError beyond W.
    shared_prefix=True (the decode kernel only; the default changes nothing): sequences that hold a prefix on the same pages - beams,
    samples of one prompt, forks behind one system prompt - are grouped from the host's books (PageTable.prefix_groups) and
    lqer_attention_q_decode_paged_shared reads every chunk of keys that lies wholly inside a group's shared pages ONCE per group
    instead of once per sequence; the same bits, row for row.  When no two sequences of the call share a chunk the plain entry runs.
    With a window in effect (the call's or the cache's) or with the prefill kernel: ValueError.  On a cache with nibble codes
    (code_bits=4) the plain entry runs whatever the groups are - the same bits."""
    if kernel not in (KERNEL_DECODE, KERNEL_PREFILL, KERNEL_AUTO):
        raise ValueError(f"attention_flexible_paged: kernel={kernel!r} - 'decode', 'prefill' or 'auto'")
    _check_layout_and_mask("attention_flexible_paged", out_layout, None, causal)
    window = _window_arg("attention_flexible_paged", window, cache.window, causal)
    seqs = list(seqs)
    if q.dim() != 4:
        raise ValueError(f"attention_flexible_paged: q {tuple(q.shape)} is not [len(seqs), h, s, d]")
    b, h, s, d = q.shape
    if kernel == KERNEL_AUTO:
        kernel = KERNEL_DECODE if s <= _ATTN_DECODE_MAX_S else KERNEL_PREFILL
    prefill = kernel == KERNEL_PREFILL
    if shared_prefix and (prefill or window is not None):
        raise ValueError("attention_flexible_paged: shared_prefix=True " + ("with the prefill kernel" if prefill else f"with window={window}")
                         + " - only the decode kernel without a window reads a shared prefix once per group")
    if not prefill and s > _ATTN_DECODE_MAX_S:
        raise ValueError(f"attention_flexible_paged: {s} query rows per head - the decode kernel over the paged cache takes up to "
                         f"{_ATTN_DECODE_MAX_S} (more: kernel='prefill')")
    if (q.dtype != cache.dtype or q.device != cache.buf.device or b != len(seqs) or b < 1 or d != cache.head_dim or h % cache.kv_heads or s < 1
            or h > _MAX_GRID_Z or (prefill and b * cache.kv_heads > _MAX_GRID_Z)):
        raise ValueError(f"attention_flexible_paged: q {tuple(q.shape)} {q.dtype} on {q.device} for {len(seqs)} sequences of a cache "
                         f"[{cache.kv_heads}, {cache.head_dim}] {cache.dtype} on {cache.buf.device}")
    try:
        slots = cache.pt.slots(seqs)
    except KeyError as e:
        raise ValueError(e.args[0]) from None
    lens = [cache.pt.lengths[x] for x in slots]
    if min(lens) < 1 or (causal and s > min(lens)) or (prefill and max(lens) > _ATTN_MAX_T):
        raise ValueError(f"attention_flexible_paged: lengths {lens} of sequences {seqs} - an empty sequence has nothing to attend to"
                         + (f", and causal needs {s} query rows <= every length" if causal else ""))
    if window is not None:
        _released_below("attention_flexible_paged", cache, slots, window)
        if prefill:
            window = _prefill_window("attention_flexible_paged", cache, seqs, slots, lens, [s] * b, window)
    if q.stride(3) != 1:
        q = q.contiguous()
    out, ob, stats = _attention_outputs(q, out_layout, return_stats)
    groups = None
    if shared_prefix:
        L = _lib.lib()
        groups = cache.pt.prefix_groups(slots, lens, lambda t: L.lqer_attention_q_decode_chunk(t, d))
    _paged_call(PAGED_PREFILL if prefill else PAGED_DECODE, q, ob, stats, cache, slots, lens, scaling, causal, ws, window, S=s, groups=groups)
    return (out, stats) if return_stats else out


PAGED_PREFILL, PAGED_DECODE = "lqer_attention_q_paged", "lqer_attention_q_decode_paged"
SHARED_DECODE = "lqer_attention_q_decode_paged_shared"
RAGGED_PREFILL, RAGGED_DECODE = "lqer_attention_q_paged_ragged", "lqer_attention_q_decode_paged_ragged"
TREE_PREFILL, TREE_DECODE = "lqer_attention_q_paged_tree", "lqer_attention_q_decode_paged_tree"
_SIBLING = {TREE_PREFILL: RAGGED_PREFILL, TREE_DECODE: RAGGED_DECODE}  # whose workspace a tree entry has
TREE_MAX_NODES = 64  # a row's mask is one 64-bit word


def _window_arg(who, window, default, causal):
    """The window a call runs under: `window` - None or a number of keys >= 1, ValueError otherwise - or, for None, `default` (the
    cache's).  A window without `causal` is refused."""
    if window is None:
        window = default
    elif not isinstance(window, int) or isinstance(window, bool) or window < 1:
        raise ValueError(f"{who}: window {window!r} - None or a number of keys >= 1")
    if window is not None and not causal:
        raise ValueError(f"{who}: window={window} without causal=True - the window is a rule on top of the causal one")
    return window


def _released_below(who, cache, slots, window) -> None:
    """An explicit window wider than the cache's cannot run on sequences that have let pages go."""
    if window is not None and any(cache.pt.released[x] for x in slots) and (cache.window is None or window > cache.window):
        raise ValueError(f"{who}: window={window} on sequences that have released the pages below the cache's window of {cache.window} keys")


def _prefill_window(who, cache, seqs, slots, lens, counts, window):
    """The window rule of ONE prefill call on sequences `seqs` (in `slots`, of `lens` keys, with `counts` query rows) under the
    effective window: None - the unwindowed entry - without a window or while every length is <= W (the rule changes nothing, and
    nothing can have been released); else W - the *_window entry -, which needs a cache made with max_query_rows and, of every
    sequence, still the page of the first key its first query row sees.  ValueError otherwise."""
    if window is None or max(lens) <= window:
        return None
    if cache.max_query_rows is None:
        raise ValueError(f"{who}: kernel='prefill' with window={window} and lengths {lens} - the prefill kernel has no window "
                         "rule on a cache made without max_query_rows; it is taken while every length is <= the window")
    for seq, x, t, c in zip(seqs, slots, lens, counts):
        if PAGE_KEYS * cache.pt.released[x] > max(0, t - c - window + 1):
            raise ValueError(f"{who}: sequence {seq} of {t} keys has released its first {cache.pt.released[x]} pages, and {c} query rows under "
                             f"window={window} start at key {max(0, t - c - window + 1)} - the keys are gone (the cache keeps them for up to "
                             f"max_query_rows = {cache.max_query_rows} rows)")
    return window


def _paged_max_len(base, cache, lens) -> int:
    """The bound handed to the library, which sizes grids and workspace: the table's room for PAGED_DECODE (as ever), for all others
    the longest addressed length rounded up to 128, capped at the room - tight, since no result depends on it."""
    return cache.pt.max_len if base == PAGED_DECODE else min((max(max(lens), 1) + 127) // 128 * 128, cache.pt.max_len)


def _paged_args(base, q, out, stats, cache: PagedKVCache, slots, lens, scaling, causal, window, ws_ptr, ws_bytes, stream, S=None, counts=None,
                groups=None, tree=None):
    """(entry, its argument tuple) for one of the ten attention entries over the pool: `base` - PAGED_* on q / out [b, h, S, d]
    (out: any strides over b, h, S), RAGGED_* / TREE_* on q / out [sum(counts), h, d] (any token and head strides) with `counts` query
    rows per sequence -, stats fp32 dense or None, for the sequences in `slots` with `lens` keys.  `window`: None or W - the entry is
    then `base`_window, but for RAGGED_DECODE, which always takes one (0: none).  `tree` (TREE_* alone, which take no window): the
    rows' masks, int64 [sum(counts)] on the device, in the last place.  `groups` (PAGED_DECODE without a window only): the call's
    prefix groups (PageTable.prefix_groups) - with a group of two or more the entry is SHARED_DECODE, `base`'s list plus the group
    arrays; with none, without any such group, or on a cache with nibble codes (the grouped kernels are not instantiated for them; the
    bits are the same), `base`.  The workspace and the stream come as values, so nothing
    here needs a GPU: the call's metadata is copied to the cache's device tensors, wherever they are."""
    ragged, f = counts is not None, cache.fmts
    h, d = q.shape[1], q.shape[-1]
    max_len = _paged_max_len(base, cache, lens)
    args = (q.data_ptr(), *cache._pool_args(), *cache._call_meta(slots, lens, max_len), out.data_ptr(),
            stats.data_ptr() if stats is not None else None, ops.dtype_code(q), len(slots), h, cache.kv_heads,
            *((cache._call_starts(counts), max(counts), q.shape[0]) if ragged else (S,)), d,
            *((_pair(q), _pair(out)) if ragged else (_tri(q), _tri(out))), float(scaling), int(bool(causal)),
            C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), C.byref(f[3]), ws_ptr, ws_bytes, stream)
    if base in _SIBLING:
        if tree is None or window is not None:
            raise ValueError(f"{base} with tree={tree!r}, window={window} - a tree entry takes the rows' masks and no window")
        return base, args + (tree.data_ptr(),)
    if base == RAGGED_DECODE:
        return base, args + (0 if window is None else min(window, 1 << 62),)
    if groups is not None and any(len(mem) > 1 for mem, _ in groups):
        if base != PAGED_DECODE or window is not None:
            raise ValueError(f"prefix groups on {base} with window={window} - {SHARED_DECODE} is {PAGED_DECODE} alone")
        if not cache.nibble:
            return SHARED_DECODE, args + cache._call_groups(groups)
    return (base, args) if window is None else (base + "_window", args + (min(window, 1 << 62),))


def _paged_call(base, q, out, stats, cache: PagedKVCache, slots, lens, scaling, causal, ws, window, S=None, counts=None, groups=None,
                tree=None) -> None:
    """The library call _paged_args describes; ws: a uint8 workspace, or None for the stream's at the size `base`_workspace_bytes asks
    (a *_window entry and a TREE_* entry have their sibling's)."""
    L = _lib.lib()
    with torch.cuda.device(q.device):
        if ws is None:
            h, d = q.shape[1], q.shape[-1]
            max_len = _paged_max_len(base, cache, lens)
            sized_by = _SIBLING.get(base, base)
            need = (L.lqer_attention_q_decode_paged_ragged_workspace_bytes(q.shape[0], h, max_len, d) if sized_by == RAGGED_DECODE else
                    getattr(L, sized_by + "_workspace_bytes")(len(slots), h, cache.kv_heads, S if counts is None else max(counts), max_len, d))
            ws = ops.workspace(q.device, max(need, 16))
        name, args = _paged_args(base, q, out, stats, cache, slots, lens, scaling, causal, window, ws.data_ptr(), ws.numel(), ops._stream(q.device),
                                 S, counts, groups, tree)
        _lib.check(getattr(L, name)(*args), name)


def _ragged_counts(who, seqs, counts):
    seqs = list(seqs)
    try:
        counts = [int(c) for c in counts]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: counts {counts!r} - one count >= 0 per sequence") from None
    if len(counts) != len(seqs) or any(c < 0 for c in counts):
        raise ValueError(f"{who}: counts {counts} for {len(seqs)} sequences - one count >= 0 per sequence")
    return seqs, counts


def _ragged_operands(who, q, cache, seqs, counts, causal):
    """What every call with per-sequence counts asks of q, the sequences and their lengths: (slots, lens), or ValueError."""
    if q.dim() != 3 or q.shape[0] != sum(counts):
        raise ValueError(f"{who}: q {tuple(q.shape)} is not [sum(counts) = {sum(counts)}, h, d]")
    total, h, d = q.shape
    if (q.dtype != cache.dtype or q.device != cache.buf.device or d != cache.head_dim or h < 1 or h % cache.kv_heads or h > _MAX_GRID_Z):
        raise ValueError(f"{who}: q {tuple(q.shape)} {q.dtype} on {q.device} for a cache [{cache.kv_heads}, {cache.head_dim}] {cache.dtype} on "
                         f"{cache.buf.device}")
    try:
        slots = cache.pt.slots(seqs)
    except KeyError as e:
        raise ValueError(e.args[0]) from None
    lens = [cache.pt.lengths[x] for x in slots]
    for seq, t, c in zip(seqs, lens, counts):
        if c and (t < 1 or (causal and c > t)):
            raise ValueError(f"{who}: sequence {seq} of {t} keys with {c} query rows - an empty sequence has nothing to attend to"
                             + (f", and causal needs {c} query rows <= the length" if causal else ""))
    return slots, lens


@torch.no_grad()
def attention_flexible_paged_decode_ragged(q, cache: PagedKVCache, seqs, counts, scaling, causal=False, return_stats=False, ws=None, window=None):
    """attention_flexible_paged(kernel="decode") for sequences with up to 8 query rows EACH, a count of its own per sequence, in ONE
    library call (lqer_attention_q_decode_paged_ragged: three launches whatever the counts are) - the verify step of a speculative
    decoder, 1 .. 8 draft tokens per sequence; a scheduler step of one-token decoders beside sequences that take a few.
    q [sum(counts), h, d]: sequence seqs[b] owns rows sum(counts[:b]) .. + counts[b] - 1; the output has q's shape, the statistics are
    [sum(counts), h, 2].  Every count is 0 .. 8; a count of 0 leaves its sequence out (it may be empty).  `causal`: key j of sequence
    b visible to its query row i iff j <= i + (length_b - counts[b]).  Every sequence gets the bits of
    attention_flexible_paged(kernel="decode") on it alone - those of attention_flexible(..., kernel="decode") on its raw K and V.
    `window` (default: the cache's; needs causal=True): the window rule per sequence, as attention_flexible_paged's - the bits of the
    decode kernel on the full raw K and V with the additive window mask, no released page read.  The workspace follows sum(counts),
    and the library's bound max_len is the longest addressed length rounded up to 128 (capped at the table's room).  ValueError before
    anything is launched: what attention_flexible_paged_ragged refuses, in its words, and a count above 8 (more rows:
    attention_flexible_paged_ragged).  ws: a uint8 workspace or None (the stream's)."""
    who = "attention_flexible_paged_decode_ragged"
    eff_window = _window_arg(who, window, cache.window, causal)
    seqs, counts = _ragged_counts(who, seqs, counts)
    if any(c > _ATTN_DECODE_MAX_S for c in counts):
        raise ValueError(f"{who}: counts {counts} - the decode kernels over the paged cache take up to {_ATTN_DECODE_MAX_S} query rows per "
                         "sequence (more: attention_flexible_paged_ragged)")
    slots, lens = _ragged_operands(who, q, cache, seqs, counts, causal)
    _released_below(who, cache, (x for x, c in zip(slots, counts) if c), eff_window)
    if q.stride(2) != 1:
        q = q.contiguous()
    total, h, d = q.shape
    out = torch.empty(total, h, d, dtype=q.dtype, device=q.device)
    stats = torch.empty(total, h, 2, dtype=torch.float32, device=q.device) if return_stats else None
    if total:
        _paged_call(RAGGED_DECODE, q, out, stats, cache, slots, lens, scaling, causal, ws, eff_window, counts=counts)
    return (out, stats) if return_stats else out


def _ragged_plan(counts, kernel, names=(RAGGED_DECODE, RAGGED_PREFILL)):
    """The library calls of attention_flexible_paged_ragged (`names`: of attention_flexible_paged_tree) for these counts, host
    arithmetic only: [(name, the indices of the call's sequences, the slice of q's rows they own - None when their rows are not one
    range and are gathered)].  kernel="auto": all sequences of up to 8 rows in one call of the decode entry names[0], all others in
    one call of the prefill entry names[1]; "prefill": all in the latter.  Returns the plan and the first row of every sequence."""
    starts = [0]  # the first row of every sequence
    for c in counts[:-1]:
        starts.append(starts[-1] + c)
    live = [b for b, c in enumerate(counts) if c]
    small = [b for b in live if counts[b] <= _ATTN_DECODE_MAX_S] if kernel == KERNEL_AUTO else []
    big = [b for b in live if counts[b] > _ATTN_DECODE_MAX_S] if kernel == KERNEL_AUTO else live
    plan = []
    for name, bs in zip(names, (small, big)):
        if bs:
            lo, hi = starts[bs[0]], starts[bs[-1]] + counts[bs[-1]]
            plan.append((name, bs, slice(lo, hi) if hi - lo == sum(counts[b] for b in bs) else None))
    return plan, starts


@torch.no_grad()
def attention_flexible_paged_ragged(q, cache: PagedKVCache, seqs, counts, scaling, causal=False, return_stats=False, ws=None, kernel=KERNEL_AUTO,
                                    window=None):
    """attention_flexible_paged for sequences with a number of query rows of their own - one scheduler step of continuous batching,
    most sequences decoding one token while a few take a prompt chunk.  q [sum(counts), h, d]: sequence seqs[b] owns rows
    sum(counts[:b]) .. + counts[b] - 1; the output has q's shape, the statistics are [sum(counts), h, 2].  `causal`: key j of sequence b
    visible to its query row i iff j <= i + (length_b - counts[b]).  A count of 0 leaves its sequence out (it may be empty).
    kernel="prefill": the whole batch in ONE lqer_attention_q_paged_ragged call - the prefill kernel takes every sequence's length
    and count from the device; each sequence gets the bits of attention_flexible(..., kernel="prefill") on its raw K and V alone.
    kernel="auto" (the default): ALL sequences of up to 8 rows go through ONE lqer_attention_q_decode_paged_ragged call - the decode
    kernels take every sequence's count from the device, whatever the distinct counts are (attention_flexible_paged_decode_ragged) -
    and all others through one lqer_attention_q_paged_ragged call: at most two library calls, and every sequence gets the bits
    attention_flexible_paged(kernel="auto") gives it alone.  A call whose sequences' rows are one range of q - the decoders named
    first and the chunks last, say - takes them as a view and writes its rows of the output in place; the rows of a call that another
    call's rows lie between are gathered and scattered by index on the device, once.  attention_flexible_paged_ragged.plan(cache,
    seqs, counts, kernel, window) names the calls without touching a device.
    `window` (default: the cache's) and every refusal are those of the route a sequence takes, in its words: the decode route has the
    window rule; the prefill call runs unwindowed while every length it addresses is <= W and, beyond, as
    lqer_attention_q_paged_ragged_window on a cache made with max_query_rows (ValueError on any other, and for a sequence whose count
    reaches below the pages it still holds - attention_flexible_paged's rule).  ValueError before anything
    is launched: len(counts) != len(seqs), a negative count, sum(counts) != q.shape[0], causal with counts[b] > length_b, an empty
    sequence with a count, an unknown or repeated sequence, a wrong dtype, device or head count.  ws: a uint8 workspace or None."""
    who = "attention_flexible_paged_ragged"
    if kernel not in (KERNEL_PREFILL, KERNEL_AUTO):
        raise ValueError(f"{who}: kernel={kernel!r} - 'prefill' or 'auto'")
    eff_window = _window_arg(who, window, cache.window, causal)
    seqs, counts = _ragged_counts(who, seqs, counts)
    slots, lens = _ragged_operands(who, q, cache, seqs, counts, causal)
    plan, starts = _ragged_plan(counts, kernel)
    live = [b for _, bs, _ in plan for b in bs]
    big = [bs for name, bs, _ in plan if name == RAGGED_PREFILL]
    big = big[0] if big else []
    _released_below(who, cache, (slots[b] for b in live), eff_window)
    big_lens, big_window = [lens[b] for b in big], None
    if big:
        big_window = _prefill_window(who, cache, [seqs[b] for b in big], [slots[b] for b in big], big_lens, [counts[b] for b in big], eff_window)
    if big and (max(big_lens) > _ATTN_MAX_T or len(big) * cache.kv_heads > _MAX_GRID_Z):
        raise ValueError(f"{who}: {len(big)} sequences of lengths {big_lens} beyond the prefill kernel's launch grid")
    windows = {RAGGED_DECODE: eff_window, RAGGED_PREFILL: big_window}  # (the prefill call while every length <= W: plain causal)
    return _ragged_calls(q, cache, slots, lens, counts, plan, starts, scaling, causal, return_stats, ws, windows)


def _ragged_calls(q, cache, slots, lens, counts, plan, starts, scaling, causal, return_stats, ws, windows, tree=None):
    """The calls of a plan (_ragged_plan) over q [sum(counts), h, d], the body of attention_flexible_paged_ragged and
    attention_flexible_paged_tree: the output and the statistics allocated, every call on its rows of q, its results at those rows.
    `windows`: the window each entry of the plan runs under; `tree`: the rows' masks, int64 [sum(counts)] on the device (they travel
    with q's rows), or None."""
    total, h, d = q.shape
    if q.stride(2) != 1:
        q = q.contiguous()
    out = torch.empty(total, h, d, dtype=q.dtype, device=q.device)
    stats = torch.empty(total, h, 2, dtype=torch.float32, device=q.device) if return_stats else None
    # At most two calls: one for the sequences of the decode route, one for all others.  A call whose sequences' rows are ONE range of q
    # (no other call's rows between them: the decoders in front and the chunks behind, say) runs on views of q and out; the rows of the
    # others are gathered and scattered by index - all of them through one index tensor, copied to the device once.
    rows, where = [], []
    for _, bs, at in plan:
        where.append(at)
        if at is None:
            mine = [r for b in bs for r in range(starts[b], starts[b] + counts[b])]
            where[-1] = (len(rows), len(rows) + len(mine))
            rows += mine
    idx = torch.tensor(rows, dtype=torch.int64).to(q.device) if rows else None
    for (name, bs, _), at in zip(plan, where):
        args = (cache, [slots[b] for b in bs], [lens[b] for b in bs], scaling, causal, ws, windows[name])
        mine = [counts[b] for b in bs]
        if isinstance(at, slice):  # (in place: nothing to copy)
            _paged_call(name, q[at], out[at], stats[at] if return_stats else None, *args, counts=mine, tree=None if tree is None else tree[at])
            continue
        ix = idx[at[0]:at[1]]
        qc = q.index_select(0, ix)
        oc = torch.empty_like(qc)
        sc = torch.empty(qc.shape[0], h, 2, dtype=torch.float32, device=q.device) if return_stats else None
        _paged_call(name, qc, oc, sc, *args, counts=mine, tree=None if tree is None else tree.index_select(0, ix))
        out.index_copy_(0, ix, oc)
        if return_stats:
            stats.index_copy_(0, ix, sc)
    return (out, stats) if return_stats else out


def _plan(cache: PagedKVCache, seqs, counts, kernel=KERNEL_AUTO, window=None) -> list:
    """The library calls attention_flexible_paged_ragged(q, cache, seqs, counts, ..., kernel=kernel, window=window) makes, in order,
    from host state alone (no device is touched): one dict per call - "call": the C entry, "seqs": the indices into `seqs` of the
    sequences it takes, "rows": "view" when their rows are one range of q and the call runs on views of q and out, "gathered" when
    they are gathered and scattered by index, "window": the window rule it runs under (None: none).  The prefill call has a rule
    only on a cache made with max_query_rows, and only when a length it addresses - read from the host's books, which then must know
    `seqs` - lies beyond the window: it is then lqer_attention_q_paged_ragged_window, by the function's own rule (_prefill_window),
    its refusal of a count that reaches below the pages a sequence still holds included.  On any other cache no length is read.  Each
    call is three launches.  Refuses an unknown `kernel`, a bad `window` and bad counts as the function does."""
    who = "attention_flexible_paged_ragged"
    if kernel not in (KERNEL_PREFILL, KERNEL_AUTO):
        raise ValueError(f"{who}: kernel={kernel!r} - 'prefill' or 'auto'")
    eff_window = _window_arg(who, window, cache.window, True)
    seqs, counts = _ragged_counts(who, seqs, counts)
    out = []
    for name, bs, at in _ragged_plan(counts, kernel)[0]:
        win = eff_window if name == RAGGED_DECODE else None
        if name == RAGGED_PREFILL and eff_window is not None and cache.max_query_rows is not None:
            mine = [seqs[b] for b in bs]
            try:
                slots = cache.pt.slots(mine)
            except KeyError as e:
                raise ValueError(e.args[0]) from None
            win = _prefill_window(who, cache, mine, slots, [cache.pt.lengths[x] for x in slots], [counts[b] for b in bs], eff_window)
            name += "_window" if win is not None else ""
        out.append({"call": name, "seqs": bs, "rows": "view" if at is not None else "gathered", "window": win})
    return out


attention_flexible_paged_ragged.plan = _plan


def tree_masks(parents) -> list:
    """One sequence's rows of a draft tree from its nodes' parents: parents[i] is -1 for a child of the committed context, else the
    index - below i: parents come before children - of node i's parent.  Row i of the result has bit j set iff node j is node i or
    one of its ancestors: what lqer_attention_q_decode_paged_tree / lqer_attention_q_paged_tree read per query row.  A chain gives
    (2 << i) - 1, the causal rule; a star 1 << i.  ValueError for more than 64 nodes, a parent at or above its node's index or below -1."""
    try:
        parents = [int(p) for p in parents]
    except (TypeError, ValueError):
        raise ValueError(f"tree_masks: parents {parents!r} - one index per node, -1 for a child of the committed context") from None
    if len(parents) > TREE_MAX_NODES:
        raise ValueError(f"tree_masks: {len(parents)} nodes - a row's mask is one 64-bit word: up to {TREE_MAX_NODES} nodes per sequence")
    masks = []
    for i, p in enumerate(parents):
        if p < -1 or p >= i:
            raise ValueError(f"tree_masks: node {i} with parent {p} - -1 (the committed context) or a node before it: parents come before children")
        masks.append((1 << i) | (masks[p] if p >= 0 else 0))
    return masks


def _tree_operands(who, cache, seqs, parents, kernel):
    """What attention_flexible_paged_tree and its .plan ask of the host arguments alone: (seqs, counts, every row's mask), or ValueError."""
    if kernel not in (KERNEL_PREFILL, KERNEL_AUTO):
        raise ValueError(f"{who}: kernel={kernel!r} - 'prefill' or 'auto'")
    if cache.window is not None:
        raise ValueError(f"{who}: a cache made with window={cache.window} - a tree row's position is its depth, not its index, so the "
                         "window rule is undefined on a draft tree")
    seqs = list(seqs)
    try:
        parents = [list(p) for p in parents]
    except TypeError:
        raise ValueError(f"{who}: parents {parents!r} - one list of parent indices per sequence") from None
    if len(parents) != len(seqs):
        raise ValueError(f"{who}: {len(parents)} parent lists for {len(seqs)} sequences - one list of parent indices per sequence")
    try:
        masks = [m for p in parents for m in tree_masks(p)]
    except ValueError as e:
        raise ValueError(f"{who}: {e.args[0]}") from None
    return seqs, [len(p) for p in parents], masks


@torch.no_grad()
def attention_flexible_paged_tree(q, cache: PagedKVCache, seqs, parents, scaling, return_stats=False, ws=None, kernel=KERNEL_AUTO):
    """The verify step of a speculative decoder that drafts a TREE (Medusa, EAGLE, SpecInfer) on paged sequences, in at most two
    library calls and without a copy of any sequence.  parents[b] lists the parents of sequence seqs[b]'s draft nodes (tree_masks:
    -1 for a child of the committed context, else an earlier node); its nodes are the LAST len(parents[b]) keys of the sequence, in
    the order they were appended (append_ragged the whole tree first), and q [sum(counts), h, d] holds their queries in that order,
    counts[b] = len(parents[b]).  Node i sees the committed context - every key before the draft - and, of the draft, itself and its
    ancestors.  The output has q's shape, the statistics are [sum(counts), h, 2].  A count of 0 leaves its sequence out.
    kernel="auto" (the default): ALL sequences of up to 8 nodes go through ONE lqer_attention_q_decode_paged_tree call, those of 9 ..
    64 nodes through ONE lqer_attention_q_paged_tree call; "prefill": all through the latter.  Rows are taken as views or gathered as
    attention_flexible_paged_ragged takes them (one body).  The masks go to the device in one copy per call.  Every sequence gets the
    bits of attention_flexible(q_b, K_b, V_b, ..., attention_mask=M, kernel="decode" / "prefill") on its raw K and V - the context
    plus ALL its draft nodes - with M = 0 where visible and torch.finfo(dtype).min elsewhere.  Sibling nodes share K quantizer blocks
    (16 keys along t), so these are not the bits of a chain verify of one path alone; the accepted path's keys get those when they
    are appended to the snapshot (PagedKVCache: "Taking speculated tokens back").
    attention_flexible_paged_tree.plan(cache, seqs, parents, kernel) names the calls without touching a device.
    ValueError before anything is launched: what attention_flexible_paged_ragged refuses, in its words (a node count above the
    sequence's length among them), more than 64 nodes, a bad parents list, a cache made with window=.  ws: a uint8 workspace or None."""
    who = "attention_flexible_paged_tree"
    seqs, counts, masks = _tree_operands(who, cache, seqs, parents, kernel)
    slots, lens = _ragged_operands(who, q, cache, seqs, counts, True)
    plan, starts = _ragged_plan(counts, kernel, (TREE_DECODE, TREE_PREFILL))
    for name, bs, _ in plan:
        if name == TREE_PREFILL and (max(lens[b] for b in bs) > _ATTN_MAX_T or len(bs) * cache.kv_heads > _MAX_GRID_Z):
            raise ValueError(f"{who}: {len(bs)} sequences of lengths {[lens[b] for b in bs]} beyond the prefill kernel's launch grid")
    # (int64 holds the 64 bits: bit 63 - row 63's own - is the sign)
    tree = torch.tensor([m - (1 << 64) if m >> 63 else m for m in masks], dtype=torch.int64).to(q.device)
    return _ragged_calls(q, cache, slots, lens, counts, plan, starts, scaling, True, return_stats, ws, {TREE_DECODE: None, TREE_PREFILL: None}, tree)


def _tree_plan(cache: PagedKVCache, seqs, parents, kernel=KERNEL_AUTO) -> list:
    """The library calls attention_flexible_paged_tree(q, cache, seqs, parents, ..., kernel=kernel) makes, in order, from host state
    alone (no device is touched, no length is read): one dict per call - "call": the C entry, "seqs": the indices into `seqs` of the
    sequences it takes, "rows": "view" or "gathered" (attention_flexible_paged_ragged.plan's words).  Each call is three launches.
    Refuses an unknown `kernel`, bad parents and a cache with a window as the function does."""
    seqs, counts, _ = _tree_operands("attention_flexible_paged_tree", cache, seqs, parents, kernel)
    return [{"call": name, "seqs": bs, "rows": "view" if at is not None else "gathered"}
            for name, bs, at in _ragged_plan(counts, kernel, (TREE_DECODE, TREE_PREFILL))[0]]


attention_flexible_paged_tree.plan = _tree_plan

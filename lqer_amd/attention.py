"""Quantized attention matmuls inside a stock HuggingFace decoder (wiring).

The reference's decoder copies replace the two matmuls of eager attention by `matmul_flexible`
(llama_decoder.py:259-297: Q K^T on [b*h, s, d] x [b*h, d, s], scaled AFTER the quantized product; softmax in fp32;
P V on [b*h, s, s] x [b*h, s, d]; opt_decoder.py:125,190 likewise with bmm).  Here the same computation is registered
as an attention implementation of the installed transformers (AttentionInterface), so no model class is copied:
`enable_quantized_attention(model, q_config)` selects it and stores the per-layer matmul configs on the attention
modules.  Operands are flattened to 3-D like the reference does (its quantizer rejects 4-D tensors); blocks run along
the last dim of each operand.
"""
from __future__ import annotations

from copy import deepcopy
from typing import Optional

import torch
import torch.nn as nn

from .functional import KERNEL_PREFILL, _ATTN_DECODE_MAX_S, _repeat_kv, attention_flexible, unfused_attention  # noqa: F401  (_repeat_kv: the one spelling, in functional)
from .kvcache import QuantizedKVCache, attention_flexible_cached

IMPLEMENTATION = "lqer_eager"
IMPLEMENTATION_FUSED = "lqer_fused"  # the same computation as ONE kernel (csrc/attn_q.hip): enable_quantized_attention(..., fused=True)


def lqer_eager_attention_forward(module: nn.Module, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                                 attention_mask: Optional[torch.Tensor], scaling: float, dropout: float = 0.0, **kwargs):
    cfg0, cfg1 = module._lqer_matmul_cfg
    out, attn_weights = unfused_attention(query, key, value, cfg0, cfg1, scaling, attention_mask, dropout=dropout, training=module.training)
    return out.transpose(1, 2).contiguous(), attn_weights


def lqer_fused_attention_forward(module: nn.Module, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                                 attention_mask: Optional[torch.Tensor], scaling: float, dropout: float = 0.0, **kwargs):
    """lqer_eager_attention_forward through attention_flexible: the mask tensor goes to the kernel as it is, grouped-query K / V
    are read through the head mapping, the output is written as [b, s, h, d] and no weights exist to return.  A caller that wants
    the weights (output_attentions), trains with dropout or hands over a mask of another dtype gets the unfused function.
    key / value that carry a packed cache layer (quantized_kv_cache below: a decode step, key and value are the NEW tokens only) run
    attention_flexible_cached over that layer's cache - more than 8 new tokens, which only a chunked_prefill layer tags, with the prefill
    kernel; there the unfused function has nothing to run on, and those callers get an error."""
    unfused = (kwargs.get("output_attentions") or (dropout > 0.0 and module.training)
               or (attention_mask is not None and attention_mask.dtype != query.dtype))  # (a wider mask: torch adds it with type promotion)
    layer = getattr(key, _KV_LAYER_ATTR, None)
    if layer is not None:
        chunk = query.shape[2] > _ATTN_DECODE_MAX_S
        if unfused or (chunk and not layer.chunked_prefill):
            raise NotImplementedError("lqer_fused attention over a packed KV cache: output_attentions, dropout in training, a mask of another "
                                      f"dtype and more than {_ATTN_DECODE_MAX_S} new tokens need the raw K and V, which the cache does not keep")
        return attention_flexible_cached(query, layer.cache, scaling, attention_mask=attention_mask, out_layout="bshd",
                                         kernel=KERNEL_PREFILL if chunk else None), None
    if unfused:
        return lqer_eager_attention_forward(module, query, key, value, attention_mask, scaling, dropout=dropout, **kwargs)
    cfg0, cfg1 = module._lqer_matmul_cfg
    out = attention_flexible(query, key, value, cfg0, cfg1, scaling, attention_mask=attention_mask, out_layout="bshd")
    return out, None


_KV_LAYER_ATTR = "_lqer_kv_layer"  # on the key / value tensors a packed cache layer's update() returns for a decode step


def _kv_layer_cls():
    """The cache layer class, made on first use (transformers is imported only where a model is at hand)."""
    global _KV_LAYER_CLS
    if _KV_LAYER_CLS is not None:
        return _KV_LAYER_CLS
    from transformers.cache_utils import CacheLayerMixin

    class QuantizedKVLayer(CacheLayerMixin):
        """One attention layer's K and V as a QuantizedKVCache.  An update() on the empty layer (the prefill) packs k and v and returns
        them as they are: the attention runs over the raw tensors, as without a cache.  An update() with up to 8 new tokens on a
        non-empty layer appends them and returns the NEW k and v tagged with this layer; lqer_fused_attention_forward then attends over
        the cache.  More new tokens on a non-empty layer raise: the raw K and V of the past are gone - unless the layer was made with
        chunked_prefill=True: then they are appended and tagged like a decode step's, and the attention over the cache is the prefill
        kernel on images written from the codes (attention_flexible_cached(kernel="prefill"))."""

        is_sliding = False

        def __init__(self, cfg0: dict, cfg1: dict, capacity: int = 256, chunked_prefill: bool = False):
            super().__init__()
            self.cfg0, self.cfg1, self.capacity0, self.chunked_prefill = cfg0, cfg1, capacity, bool(chunked_prefill)
            self.cache: Optional[QuantizedKVCache] = None

        def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
            b, hk, _, d = key_states.shape
            self.dtype, self.device = key_states.dtype, key_states.device
            self.cache = QuantizedKVCache(b, hk, d, self.cfg0, self.cfg1, self.dtype, self.device, capacity=self.capacity0)
            self.is_initialized = True

        def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
            if not self.is_initialized:
                self.lazy_initialization(key_states, value_states)
            past, n = self.cache.length, key_states.shape[-2]
            if past > 0 and n > _ATTN_DECODE_MAX_S and not self.chunked_prefill:
                raise NotImplementedError(f"packed KV cache: {n} new tokens on a cache of {past} - the kernel over the cache takes up to "
                                          f"{_ATTN_DECODE_MAX_S} query rows, and the raw K and V of the past are not kept (no chunked prefill)")
            self.cache.append(key_states, value_states)
            if past > 0:
                setattr(key_states, _KV_LAYER_ATTR, self)
                setattr(value_states, _KV_LAYER_ATTR, self)
            return key_states, value_states

        def get_mask_sizes(self, query_length: int) -> tuple:
            return self.get_seq_length() + query_length, 0

        def get_seq_length(self) -> int:
            return self.cache.length if self.cache is not None else 0

        def get_max_length(self) -> int:
            return -1

        @property
        def nbytes(self) -> int:
            return self.cache.nbytes if self.cache is not None else 0

        def reset(self) -> None:
            if self.cache is not None:
                self.cache.reset()

        def _no(self, what):
            raise NotImplementedError(f"packed KV cache: {what} is not implemented")

        def offload(self):
            self._no("offloading")

        def prefetch(self):
            pass

        def _select(self, indices) -> None:  # (a layer not yet initialised has no batch: the first update() brings it)
            if self.cache is not None:
                self.cache.select(indices)

        def reorder_cache(self, beam_idx) -> None:
            self._select(beam_idx)

        def crop(self, *args, **kwargs) -> None:
            self._no("crop")

        def batch_repeat_interleave(self, repeats: int) -> None:
            if self.cache is not None:
                self._select(torch.arange(self.cache.batch).repeat_interleave(repeats))

        def batch_select_indices(self, indices) -> None:
            self._select(indices)

    _KV_LAYER_CLS = QuantizedKVLayer
    return QuantizedKVLayer


_KV_LAYER_CLS = None


def quantized_kv_cache(model: nn.Module, capacity: int = 256, chunked_prefill: bool = False):
    """A transformers.Cache for `model` (after enable_quantized_attention(model, q_config, fused=True)) whose layers hold K and V as
    the codes of that layer's two matmul configs (QuantizedKVCache): pass it as past_key_values to forward() or generate().  The
    decode steps give the bits of a DynamicCache run that takes the decode kernel.  Llama-family and OPT attention hand update()'s
    tensors to the attention interface untouched, which is what carries the layer to lqer_fused_attention_forward.
    chunked_prefill=True: the layers also take more than 8 new tokens on a non-empty cache (a second turn, a long prompt in chunks, a
    speculated block) - the prefill kernel over the cache, with the bits of a DynamicCache run that takes the prefill kernel on the raw K
    and V.  The default keeps the NotImplementedError for such a call."""
    from transformers.cache_utils import Cache

    from .models import _decoder_layers

    impl = getattr(getattr(model, "config", None), "_attn_implementation", None)
    if impl != IMPLEMENTATION_FUSED:
        raise ValueError(f"quantized_kv_cache: the model's attention implementation is {impl!r}, not {IMPLEMENTATION_FUSED!r} - only the fused "
                         "kernel reads the packed cache (enable_quantized_attention(model, q_config, fused=True))")
    layers, _ = _decoder_layers(model)
    cls, out = _kv_layer_cls(), []
    for i, layer in enumerate(layers):
        attn = layer.self_attn
        cfg0, cfg1 = attn._lqer_matmul_cfg
        head_dim = int(getattr(attn, "head_dim"))
        if not QuantizedKVCache.covers(cfg0, cfg1, head_dim, model.dtype):
            raise NotImplementedError(f"quantized_kv_cache: layer {i} (head_dim {head_dim}, {model.dtype}) has matmul quantizers outside the packed "
                                      "cache: block_fp, width <= 8, blocks of 16; head dims that are multiples of 16 up to 128")
        out.append(cls(cfg0, cfg1, capacity, chunked_prefill))
    return Cache(layers=out)


def _register() -> None:
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, eager_mask

    AttentionInterface.register(IMPLEMENTATION, lqer_eager_attention_forward)
    AttentionMaskInterface.register(IMPLEMENTATION, eager_mask)
    AttentionInterface.register(IMPLEMENTATION_FUSED, lqer_fused_attention_forward)
    AttentionMaskInterface.register(IMPLEMENTATION_FUSED, eager_mask)


def enable_quantized_attention(model: nn.Module, q_config: dict, fused: bool = False) -> nn.Module:
    """Route every decoder layer's attention through matmul_flexible.  q_config["matmul"] applies to both products of
    every layer unless `model_layer_<i>` / `model_layer` carry `self_attn: {matmul_0, matmul_1}` overrides
    (llama_decoder.py:423-482); OPT models read q_config["bmm"] and `bmm_0` / `bmm_1` instead, as the reference's OPT
    decoder does (opt_decoder.py:125,190,329-339).  Model families without the attention-interface hook raise.
    `fused=True` selects the implementation "lqer_fused": the whole attention as one HIP kernel where the quantizers and the head
    dim allow it (functional.attention_flexible), the unfused sequence - with its results - where they do not."""
    from .models import _OPT, _decoder_layers

    _register()
    layers, table = _decoder_layers(model)
    op = "bmm" if table is _OPT else "matmul"
    base = q_config[op]
    for i, layer in enumerate(layers):
        attn = layer.self_attn
        cfgs = []
        for name in (f"{op}_0", f"{op}_1"):
            cfg = base
            for key in (f"model_layer_{i}", "model_layer"):
                entry = q_config.get(key)
                if entry is not None and name in entry.get("self_attn", {}):
                    cfg = entry["self_attn"][name]
                    break
            cfgs.append(deepcopy(cfg))
        attn._lqer_matmul_cfg = tuple(cfgs)
    if not hasattr(model, "set_attn_implementation"):
        raise NotImplementedError(f"{type(model).__name__}: no attention-implementation switch in this transformers version")
    model.set_attn_implementation(IMPLEMENTATION_FUSED if fused else IMPLEMENTATION)
    return model

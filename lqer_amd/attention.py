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

from .functional import _repeat_kv, attention_flexible, unfused_attention  # noqa: F401  (_repeat_kv: the one spelling, in functional)

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
    the weights (output_attentions), trains with dropout or hands over a mask of another dtype gets the unfused function."""
    if (kwargs.get("output_attentions") or (dropout > 0.0 and module.training)
            or (attention_mask is not None and attention_mask.dtype != query.dtype)):  # (a wider mask: torch adds it with type promotion)
        return lqer_eager_attention_forward(module, query, key, value, attention_mask, scaling, dropout=dropout, **kwargs)
    cfg0, cfg1 = module._lqer_matmul_cfg
    out = attention_flexible(query, key, value, cfg0, cfg1, scaling, attention_mask=attention_mask, out_layout="bshd")
    return out, None


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

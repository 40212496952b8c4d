"""Model-swap helper: put the HIP quantized Linear into a stock HuggingFace decoder.

Counterpart of the reference's `quantize_model` (src/lqer/models/__init__.py:21) and of the wiring in
`run_evaluate_perplexity` (src/lqer/runners.py:212-222).  The reference copies whole decoder-layer classes
with the Linear constructor swapped (llama_decoder.py:62-145, opt_decoder.py:21-236) and reloads the
original weights with strict=False (llama_decoder.py:494-508); here the `nn.Linear` children of every
decoder layer are replaced *by name*, which yields the same module paths and therefore the same state-dict
keys (`model.layers.<i>.self_attn.q_proj.{weight,A,B}` ...), so HF checkpoints and the reference's
`low_rank_dict.pt` load unchanged.  Works with whatever transformers version is installed.

Config expansion follows llama_decoder.py:423-482: `q_config["linear"]` / `l_config["linear"]` apply to every
projection of every layer unless a `model_layer_<i>` entry overrides them.  The attention matmuls
(`q_config["matmul"]`, reference quantized_functions/matmul.py) are switched on separately:
lqer_amd.attention.enable_quantized_attention.
"""
from __future__ import annotations

from copy import deepcopy
from typing import Dict, Iterable, Optional, Tuple

import torch
import torch.nn as nn

from .linear import LinearFlexibleLqer, SharedActivation, get_quantized_layer_cls

# decoder-layer children that the reference quantizes, by model family
_LLAMA_LIKE = {"self_attn": ("q_proj", "k_proj", "v_proj", "o_proj"), "mlp": ("gate_proj", "up_proj", "down_proj")}
_OPT = {"self_attn": ("q_proj", "k_proj", "v_proj", "out_proj"), "": ("fc1", "fc2")}


def _decoder_layers(model: nn.Module) -> Tuple[nn.ModuleList, Dict[str, Tuple[str, ...]]]:
    base = getattr(model, "model", model)
    if hasattr(base, "layers"):  # Llama / Mistral (llama_decoder.py:494, mistral_decoder.py:594)
        return base.layers, _LLAMA_LIKE
    if hasattr(base, "decoder") and hasattr(base.decoder, "layers"):  # OPT (opt_decoder.py:383)
        return base.decoder.layers, _OPT
    raise ValueError(f"unsupported model class {type(model).__name__}: no decoder layer list found")


def _layer_cfg(cfg: Optional[dict], layer_id: int, group: str, name: str) -> Optional[dict]:
    """Per-projection config: `model_layer_<i>` override, else the `model_layer` template, else `linear`."""
    if cfg is None:
        return None
    for key in (f"model_layer_{layer_id}", "model_layer"):
        entry = cfg.get(key)
        if entry is not None:
            node = entry.get(group, entry) if group else entry
            if name in node:
                return deepcopy(node[name])
    return deepcopy(cfg["linear"])


# projections of one decoder layer that are fed the same tensor (llama_decoder.py:246-248 q/k/v, :176 gate/up;
# opt_decoder.py q/k/v)
_SHARED_INPUTS = {"self_attn": (("q_proj", "k_proj", "v_proj"),), "mlp": (("gate_proj", "up_proj"),)}


class _ActInFront(LinearFlexibleLqer):
    """OPT's fc2 under fuse_mlp: the layer's activation_fn is an identity and this Linear applies relu inside its activation side."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_gated(x, None, "relu")


def _gated_mlp_forward(self, x):
    return self.down_proj.forward_gated(self.gate_proj(x), self.up_proj(x), self._lqer_act)


_FUSED_MLP_CLS: Dict[type, type] = {}


def _fuse_mlp(model: nn.Module, layer: nn.Module, table: dict) -> None:
    """One decoder layer's MLP -> gate / up through their projections, then down_proj.forward_gated(g, u) (Llama-like: the mlp's class
    becomes a subclass whose forward is that statement - no module is added, state-dict keys stay, deep copies keep working);
    OPT: activation_fn becomes an identity and fc2 applies the relu itself."""
    llama = table is _LLAMA_LIKE
    act = getattr(model.config, "hidden_act" if llama else "activation_function", None)
    if act not in (("silu", "relu") if llama else ("relu",)):
        raise NotImplementedError(f"fuse_mlp: activation {act!r} is not served by forward_gated ({'silu, relu' if llama else 'relu'})")
    if llama:
        mlp = layer.mlp
        if not isinstance(mlp.down_proj, LinearFlexibleLqer):  # (a per-layer override to a plain LinearFlexible: left as it is)
            return
        cls = type(mlp)
        if cls not in _FUSED_MLP_CLS:
            _FUSED_MLP_CLS[cls] = type("Gated" + cls.__name__, (cls,), {"forward": _gated_mlp_forward})
        mlp._lqer_act = act
        mlp.__class__ = _FUSED_MLP_CLS[cls]
    elif type(layer.fc2) is LinearFlexibleLqer:
        layer.fc2.__class__ = _ActInFront
        layer.activation_fn = nn.Identity()


def _fused_norm_forward(self, hidden_states):
    """The RMSNorm in front of a SharedActivation group under fuse_norm: where the group's next round will run the fused-norm kernel the
    RAW hidden state is handed on (the group is armed with it, its version, the weight and eps, and forms the norm inside its quantizer
    launch); everywhere else the original norm runs."""
    g, w = self._lqer_group, self.weight
    if (g is not None and w.dtype == hidden_states.dtype and w.device == hidden_states.device and w.is_contiguous()
            and w.data_ptr() % 16 == 0 and g.normed_serves(hidden_states)):
        g.arm_normed(hidden_states, w, self.variance_epsilon)
        return hidden_states
    return type(self).__mro__[1].forward(self, hidden_states)


_FUSED_NORM_CLS: Dict[type, type] = {}
_NORM_IN_FRONT = {"input_layernorm": ("self_attn", "q_proj"), "post_attention_layernorm": ("mlp", "gate_proj")}


def _fuse_norm(layer: nn.Module, table: dict) -> None:
    """One decoder layer's two norms -> a subclass whose forward arms the group behind it (no module is added, state-dict keys stay,
    deep copies keep working).  Only weight * (x * rsqrt(mean x^2 + eps)) is served: HF's LlamaRMSNorm / MistralRMSNorm."""
    if table is not _LLAMA_LIKE:
        raise NotImplementedError("fuse_norm: OPT's LayerNorm is not of the form weight * (x * rsqrt(mean x^2 + eps)); not served "
                                  "(fuse_layernorm=True serves it)")
    for name, (parent, first) in _NORM_IN_FRONT.items():
        norm = getattr(layer, name, None)
        form = (norm is not None and not isinstance(norm, nn.LayerNorm) and type(norm).__name__.endswith("RMSNorm")
                and not type(norm).__name__.startswith("Gemma") and isinstance(getattr(norm, "weight", None), nn.Parameter)
                and hasattr(norm, "variance_epsilon") and getattr(norm, "bias", None) is None)
        if not form:
            raise NotImplementedError(f"fuse_norm: {name} ({type(norm).__name__}) is not of the form weight * (x * rsqrt(mean x^2 + eps)) "
                                      "(LlamaRMSNorm / MistralRMSNorm); LayerNorm and 1 + weight norms are not served")
        group = getattr(getattr(getattr(layer, parent), first), "_group", None)
        if group is None:  # (no enabled group behind this norm: left as it is)
            continue
        cls = type(norm)
        if cls not in _FUSED_NORM_CLS:
            _FUSED_NORM_CLS[cls] = type("Fused" + cls.__name__, (cls,), {"forward": _fused_norm_forward})
        norm.__dict__["_lqer_group"] = group
        norm.__class__ = _FUSED_NORM_CLS[cls]


def _fused_layernorm_forward(self, hidden_states):
    """The LayerNorm in front of OPT's q/k/v group or of fc1 under fuse_layernorm: the RAW hidden state is handed on and the consumer is
    armed with it, the weight, the bias and eps.  A group must answer first that its round will run the fused kernel (its members take
    whatever tensor they are handed for x); a lone Linear computes the norm with torch itself where the kernel does not serve the call."""
    c, w, b, h = self._lqer_consumer, self.weight, self.bias, hidden_states
    if (len(self.normalized_shape) == 1 and h.is_cuda and w.dtype == h.dtype == b.dtype and w.device == h.device == b.device
            and (isinstance(c, LinearFlexibleLqer) or (all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (w, b))
                                                       and c.normed_serves(h, layer_norm=True)))):
        c.arm_layer_normed(h, w, b, self.eps)
        return h
    return nn.LayerNorm.forward(self, h)


class _FusedLayerNorm(nn.LayerNorm):
    forward = _fused_layernorm_forward


_LAYERNORM_IN_FRONT = {"self_attn_layer_norm": ("self_attn", "q_proj"), "final_layer_norm": ("", "fc1")}


def _fuse_layernorm(model: nn.Module, layer: nn.Module, table: dict) -> None:
    """One OPT decoder layer's two LayerNorms -> _FusedLayerNorm (a class swap: no module is added, state-dict keys stay, deep copies
    keep working): self_attn_layer_norm arms the q/k/v group, final_layer_norm arms fc1."""
    if table is not _OPT:
        raise NotImplementedError("fuse_layernorm: serves OPT's LayerNorm in front of q/k/v and fc1; a Llama-like model's RMSNorm is "
                                  "fuse_norm=True's")
    if not getattr(layer, "do_layer_norm_before", getattr(model.config, "do_layer_norm_before", True)):
        raise NotImplementedError("fuse_layernorm: do_layer_norm_before=False (OPT-350m) applies the norms behind the residual additions, "
                                  "not in front of a Linear")
    for name, (parent, first) in _LAYERNORM_IN_FRONT.items():
        norm = getattr(layer, name, None)
        if type(norm) not in (nn.LayerNorm, _FusedLayerNorm) or norm.weight is None or norm.bias is None:
            raise NotImplementedError(f"fuse_layernorm: {name} ({type(norm).__name__}) is not an nn.LayerNorm with weight and bias")
        lin = getattr(getattr(layer, parent) if parent else layer, first)
        consumer = lin if not parent else getattr(lin, "_group", None)
        if not isinstance(consumer, (LinearFlexibleLqer, SharedActivation)):  # (no enabled group / a plain LinearFlexible: left as it is)
            continue
        norm.__dict__["_lqer_consumer"] = consumer
        norm.__class__ = _FusedLayerNorm


def quantize_model(model: nn.Module, q_config: dict, l_config: Optional[dict], share_inputs: bool = True,
                   weight_image: str = "standard", fuse_mlp: bool = False, fuse_norm: bool = False,
                   fuse_layernorm: bool = False) -> nn.Module:
    """Replace the projections of every decoder layer in place; weights are carried over.  share_inputs: projections
    fed by the same tensor quantize it once and share one side GEMM (linear.SharedActivation); per-projection results
    are unchanged up to the fp32 summation order of the side product.  weight_image: "narrow" makes every projection keep the
    compact image of its 2- / 3-bit block_fp weight (linear._LinearBase.weight_image; a projection it does not serve raises when
    it packs).  fuse_mlp: the activation between the MLP's projections runs inside the down projection's activation-side kernel
    (linear._LinearBase.forward_gated: silu(gate) * up for Llama-like layers, relu for OPT's fc2) instead of as torch launches.  fuse_norm: the RMSNorm in front of
    q/k/v and of gate/up (Llama-like layers with share_inputs) runs inside the group's quantizer launch (csrc/act_normed.hip) from
    linear._LinearBase.normed_min_m tokens on - the normalised tensor is never written - and, up to 8 tokens, inside the group's one-launch
    decode kernel (linear.SharedActivation.decode_normed / decode_layer_normed, _LinearBase.decode_layer_normed for fc1); other norms raise
    NotImplementedError.
    fuse_layernorm: the same for an OPT layer's LayerNorms (do_layer_norm_before): self_attn_layer_norm inside the q/k/v group's
    quantizer launch, final_layer_norm inside fc1's, from the layer_normed_min_m tokens of linear.SharedActivation / _LinearBase on."""
    layers, table = _decoder_layers(model)
    for layer_id, layer in enumerate(layers):
        for group, names in table.items():
            parent = getattr(layer, group) if group else layer
            for name in names:
                old = getattr(parent, name)
                if not isinstance(old, nn.Linear):
                    raise TypeError(f"layer {layer_id} {group}.{name} is {type(old).__name__}, expected nn.Linear")
                qc = _layer_cfg(q_config, layer_id, group, name)
                lc = _layer_cfg(l_config, layer_id, group, name)
                cls = get_quantized_layer_cls("linear", qc)
                new = cls(old.in_features, old.out_features, bias=old.bias is not None, q_config=qc, l_config=lc)
                new.to(device=old.weight.device, dtype=old.weight.dtype)
                new.load_state_dict(old.state_dict(), strict=False)  # A, B stay zero until loaded
                new.weight_image = weight_image
                setattr(parent, name, new)
            if share_inputs:
                for names2 in _SHARED_INPUTS.get(group, ()):
                    mods = [getattr(parent, n, None) for n in names2]
                    if all(isinstance(m, LinearFlexibleLqer) for m in mods):
                        SharedActivation(mods)
        if fuse_mlp:
            _fuse_mlp(model, layer, table)
        if fuse_norm:
            _fuse_norm(layer, table)
        if fuse_layernorm:
            _fuse_layernorm(model, layer, table)
    return model


def load_low_rank_dict(model: nn.Module, low_rank_dict: Dict[str, torch.Tensor]) -> Iterable[str]:
    """`low_rank_dict.pt` -> the A / B parameters (runners.py:220-222: cast to the model dtype, strict=False).
    Returns the keys that did not match any parameter."""
    p = next(iter(model.parameters()))
    sd = {k: v.to(dtype=p.dtype) for k, v in low_rank_dict.items()}
    missing_ok = model.load_state_dict(sd, strict=False)
    return list(missing_ok.unexpected_keys)

"""The fused-LayerNorm entries of the C ABI (csrc/act_normed.hip, NORM_LAYER) without a GPU: declared, exported and bound, additive to
ABI 14; the refusals that are new or that sharing the checks could have lost; the models quantize_model(fuse_layernorm=True) refuses."""
import ctypes as C
import os
import re

import pytest

from bench import MXINT_Q, OPT_Q
from lqer_amd import LinearFlexibleLqer, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
NAMES = ("lqer_quantize_act_xa_layernormed", "lqer_linear_forward_layernormed")


def test_exports_declared_exported_bound():
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\s*\(" % name, hdr)
        getattr(_lib.lib(), name)
    assert _lib.lib().lqer_version() == 14 == _lib.ABI_VERSION  # additive exports
    # the forward takes lqer_linear_forward's operands behind (desc, h, norm_weight, norm_bias, eps, dtype, M, ld_h)
    assert _lib.SIGNATURES[NAMES[1]][1][8:] == _lib.SIGNATURES["lqer_linear_forward"][1][5:]


@pytest.mark.parametrize("entry", ["act", "forward"])
@pytest.mark.parametrize("kwargs, want, text", [
    (dict(nb=None), E_INVALID, "null norm bias"),
    (dict(nb=0x280004), E_UNSUPPORTED, "norm bias must be 16-byte aligned"),
    (dict(dtype=_lib.F32), E_UNSUPPORTED, "fp32 h"),
    (dict(K=8208), E_UNSUPPORTED, "above 8192"),
    (dict(x_block=32), E_UNSUPPORTED, "blocks of 16"),
    (dict(a_limbs=1), E_INVALID, "a_limbs 1"),
])
def test_refusals_before_any_gpu_call(entry, kwargs, want, text):
    """The pointers are made up: a call that got past validation would fault, one refused in time returns its code and a text."""
    K, nb, dtype, x_block, a_limbs = (kwargs.get(k, v) for k, v in dict(K=512, nb=0x280000, dtype=_lib.F16, x_block=16, a_limbs=-2).items())
    desc = LinearFlexibleLqer(K, 256, bias=False, q_config=MXINT_Q, l_config={"rank": 32})._desc()
    desc.x_fmt.block = x_block
    L = _lib.lib()
    lead = (C.byref(desc), 0x100000, 0x200000, nb, 1e-5, dtype, 8, K)
    rc = (L.lqer_quantize_act_xa_layernormed(*lead, 0x300000, a_limbs, 0x400000, 0x500000, None) if entry == "act" else
          L.lqer_linear_forward_layernormed(*lead, 0x600000, 0x300000, 0x700000, a_limbs, 1, None, 0x800000, 256, 0x400000, 1 << 30, None))
    msg = L.lqer_last_error().decode()
    assert rc == want and text in msg and "layernormed" in msg, (rc, msg)


@pytest.mark.parametrize("family", ["llama", "opt_norm_after"])
def test_fuse_layernorm_refuses_what_it_does_not_serve(family):
    import test_model_swap as T
    from lqer_amd.models import quantize_model
    from transformers import OPTConfig, OPTForCausalLM

    model, qc = T._tiny_llama(), MXINT_Q
    if family != "llama":  # (OPT-350m's layout)
        model, qc = OPTForCausalLM(OPTConfig(hidden_size=128, ffn_dim=256, num_hidden_layers=1, num_attention_heads=4, vocab_size=200,
                                             max_position_embeddings=64, word_embed_proj_dim=128, do_layer_norm_before=False)), OPT_Q
    with pytest.raises(NotImplementedError, match="^fuse_layernorm:"):
        quantize_model(model, {"linear": qc}, {"linear": {"rank": 16}}, fuse_layernorm=True)

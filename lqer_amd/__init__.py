"""lqer_amd - MI355X (gfx950) implementation of the LQER quantized-Linear inference path.

Public surface mirrors the reference's `lqer.quantize` package for this path:
    get_quantized_layer_cls("linear", q_config) -> LinearFlexible | LinearFlexibleLqer
    get_quantized_func("matmul" | "bmm", q_config) -> matmul_flexible | bmm_flexible
All compute is in liblqer_hip.so (hand-written HIP); see include/lqer_hip.h and DESIGN.md.
"""
from .functional import attention_flexible, bmm_flexible, get_quantized_func, matmul_flexible  # noqa: F401
from .kvcache import QuantizedKVCache, attention_flexible_cached  # noqa: F401
# (importable from the package; __all__ below is pinned by tests/test_kv_prefill_cpu.py and stays as it is)
from .kvcache import PagedKVCache, attention_flexible_paged, attention_flexible_paged_ragged  # noqa: F401
from .kvcache import attention_flexible_paged_decode_ragged  # noqa: F401
from .kvcache import attention_flexible_paged_tree, tree_masks  # noqa: F401
# sequences out of a paged pool and into one: export / adopt / swap_out / swap_in / adopt_from (csrc/kv_cache.hip: k_kv_pool_copy)
from .kvcache import KVPoolImage  # noqa: F401
from .linear import LinearFlexible, LinearFlexibleLqer, get_quantized_layer_cls  # noqa: F401

__all__ = ["LinearFlexible", "LinearFlexibleLqer", "get_quantized_layer_cls", "matmul_flexible", "bmm_flexible",
           "attention_flexible", "get_quantized_func", "QuantizedKVCache", "attention_flexible_cached"]

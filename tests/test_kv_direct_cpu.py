"""lqer_attention_q_paged_direct (the prefill kernel that reads the pool's codes in its key loop; kernel="direct"), the part that needs
no GPU: what the entry adds to the siblings' refusals comes with its code and a message before anything touches a device, Python
refuses the same, .plan names the one call, and the workspace is 0 bytes."""
import ctypes as C

import pytest
import torch

from lqer_amd import _lib, attention_flexible_paged_ragged, attention_flexible_paged_tree
from test_kv_nibble_cpu import C4, fmt
from test_kv_nibble_cpu import _host_cache as _nibble_cache
from test_kv_paged_cpu import E_INVALID, E_UNSUPPORTED, _fmt
from test_kv_ragged_cpu import _host_cache, pair

DIRECT = "lqer_attention_q_paged_direct"


def _attend(window=0, tree=None, causal=1, fmts=None, ws=None, ws_bytes=0, max_s=8, total=9, batch=2):
    """The entry on made-up pointers: a call that got past validation would fault, one refused in time returns its code and a text."""
    L = _lib.lib()
    fmts = fmts or [_fmt()] * 4
    st = pair(4 * 64, 64)
    rc = L.lqer_attention_q_paged_direct(0x10000, 0x100000, 1 << 24, 8, 4, 0x200000, 4, 0x300000, 0x400000, 64, 0x40000, None, _lib.F16, batch, 4, 4,
                                         0x500000, max_s, total, 64, st, st, 0.125, causal, *[C.byref(f) for f in fmts], ws, ws_bytes, None, window,
                                         tree)
    return rc, L.lqer_last_error().decode()


@pytest.mark.parametrize("case, kwargs, want, words", [
    ("nibble K codes", dict(fmts=[_fmt(), fmt(C4), _fmt(), _fmt()]), E_UNSUPPORTED, "nibble"),
    ("nibble V codes", dict(fmts=[_fmt(), _fmt(), _fmt(), fmt(C4)]), E_UNSUPPORTED, "nibble"),
    ("window with tree", dict(window=16, tree=0x600000), E_INVALID, "window"),
    ("window without causal", dict(window=16, causal=0), E_INVALID, "causal"),
    ("tree without causal", dict(tree=0x600000, causal=0), E_INVALID, "causal"),
    ("negative window", dict(window=-1), E_INVALID, "window"),
    ("65 nodes", dict(tree=0x600000, max_s=65, total=66), E_INVALID, "up to 64"),
])
def test_refusals_before_any_gpu_call(case, kwargs, want, words):
    rc, msg = _attend(**kwargs)
    assert rc == want and msg.startswith("attention_q_paged_direct:") and words in msg, (case, rc, msg)


def test_no_workspace_and_nothing_to_do():
    L = _lib.lib()
    assert L.lqer_attention_q_paged_direct_workspace_bytes(2, 4, 4, 8, 64, 64) == 0
    assert L.lqer_attention_q_paged_direct_workspace_bytes(64, 32, 8, 2048, 1 << 20, 128) == 0
    # NULL and 0 bytes pass the check: with nothing to do the call is LQER_OK, with or without a rule
    assert _attend(batch=0)[0] == 0 and _attend(total=0)[0] == 0 and _attend(total=0, window=16)[0] == 0 and _attend(total=0, tree=0x600000, max_s=64)[0] == 0
    assert _lib.SIGNATURES[DIRECT][1] == _lib.SIGNATURES["lqer_attention_q_paged_ragged"][1] + [C.c_int64, C.c_void_p]


def test_python_refuses_and_plans_from_host_state_alone():
    q = lambda n: torch.zeros(n, 4, 16, dtype=torch.float16)
    chain = lambda n: list(range(-1, n - 1))
    cache = _host_cache(12, 4, None, max_pages_per_seq=6)
    # one call for a mixed set of counts, 1 .. 8 included; the rows in order are a view
    plan = attention_flexible_paged_ragged.plan(cache, [10, 11, 12, 13, 14], [1, 8, 9, 64, 0], "direct")
    assert plan == [{"call": DIRECT, "seqs": [0, 1, 2, 3], "rows": "view", "window": None}]
    assert attention_flexible_paged_tree.plan(cache, [10, 11, 12], [chain(1), chain(26), chain(8)], "direct") == [{"call": DIRECT, "seqs": [0, 1, 2], "rows": "view"}]
    for call in (lambda: attention_flexible_paged_ragged.plan(cache, [1], [3], "flash"),
                 lambda: attention_flexible_paged_ragged(q(3), cache, [cache.alloc()], [3], 0.25, kernel="direct", window=4),  # (no causal)
                 lambda: attention_flexible_paged_tree.plan(_host_cache(12, 4, 16, max_pages_per_seq=6), [1], [chain(2)], "direct")):  # window with tree
        with pytest.raises(ValueError):
            call()
    nibble, (parent, *_) = _nibble_cache(4)
    for call in (lambda: attention_flexible_paged_ragged(q(3), nibble, [parent], [3], 0.25, causal=True, kernel="direct"),
                 lambda: attention_flexible_paged_ragged.plan(nibble, [parent], [3], "direct"),
                 lambda: attention_flexible_paged_tree(q(3), nibble, [parent], [chain(3)], 0.25, kernel="direct")):
        with pytest.raises(ValueError, match="code_bits=4"):
            call()

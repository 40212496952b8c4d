"""Sliding-window prefill over the paged KV pool (lqer_attention_q_paged_window, lqer_attention_q_paged_ragged_window: k_attn_q's WIN
instantiation of csrc/attn_q.hip on images csrc/kv_cache.hip writes under the window; lqer_amd.kvcache.PagedKVCache(max_query_rows=...)),
the part that needs no GPU: the exports are declared, exported and bound - additive, the ABI version stays -, the C refusals come with
their code and a message before anything touches a device, and the release rule with R query rows keeps its two promises: at most
(W + R + 29) // 16 pages per sequence, and the page of the first key a later call of up to R rows sees."""
import ctypes as C
import os
import random
import re

import pytest
import torch

import test_kv_window_cpu as WC
from lqer_amd import _lib
from lqer_amd.kvcache import PAGE_KEYS, attention_flexible_paged, attention_flexible_paged_ragged

ROOT = WC.ROOT
E_INVALID, E_UNSUPPORTED = -1, -2
PAIRS = {"lqer_attention_q_paged_window": "lqer_attention_q_paged", "lqer_attention_q_paged_ragged_window": "lqer_attention_q_paged_ragged"}


@pytest.mark.parametrize("name", list(PAIRS))
def test_exports_declared_exported_bound(name):
    with open(os.path.join(ROOT, "include", "lqer_hip.h")) as fh:
        hdr = fh.read()
    assert name in _lib.SIGNATURES
    getattr(_lib.lib(), name)
    ver = int(re.search(r"#define LQER_ABI_VERSION (\d+)", hdr).group(1))
    assert _lib.lib().lqer_version() == ver == _lib.ABI_VERSION == 14  # additive exports: every sibling's test pins the version they left
    # the unwindowed sibling's argument list plus the window, in the binding and in the header
    res, args = _lib.SIGNATURES[PAIRS[name]]
    assert _lib.SIGNATURES[name] == (res, args + [C.c_int64])
    decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr).group(1)
    base = re.search(r"\bint %s\s*\(([^;]*)\);" % PAIRS[name], hdr).group(1)
    norm = lambda s: " ".join(s.split())
    assert norm(decl) == norm(base) + ", int64_t window"
    # both reuse the workspace function of the sibling: there is none of their own
    assert name + "_workspace_bytes" not in _lib.SIGNATURES and name + "_workspace_bytes" not in hdr


def _attend(name, window, causal=1, q=0x10000, pool=0x100000, pool_bytes=1 << 24, pages=8, slots=4, tbl=0x200000, stride=4, seq_slots=0x300000,
            lens=0x400000, max_len=64, out=0x40000, ws=0x50000, ws_bytes=1 << 20, batch=2, heads=4, kv=4, S=12, D=64, fmts=None, starts=0x500000):
    """The made-up pointers of test_kv_window_cpu: a call that got past the checks would fault."""
    L = _lib.lib()
    fmts = fmts or [WC._fmt()] * 4
    tail = (0.125, causal, *[C.byref(f) for f in fmts], ws, ws_bytes, None, window)
    head = (q, pool, pool_bytes, pages, slots, tbl, stride, seq_slots, lens, max_len, out, None, _lib.F16, batch, heads, kv)
    if name.endswith("ragged_window"):
        st = (C.c_int64 * 2)(heads * D, D)
        rc = getattr(L, name)(*head, starts, S, batch * S, D, st, st, *tail)
    else:
        st = (C.c_int64 * 3)(heads * S * D, S * D, D)
        rc = getattr(L, name)(*head, S, D, st, st, *tail)
    return rc, L.lqer_last_error().decode()


WS_OK = _lib.lib().lqer_attention_q_paged_workspace_bytes(2, 4, 4, 12, 64, 64)


@pytest.mark.parametrize("name", list(PAIRS))
@pytest.mark.parametrize("case, kwargs, want, word", [
    # the window's own, in the words of the decode entry
    ("window = 0", dict(window=0), E_INVALID, "a sliding window is W >= 1 keys on top of the causal rule"),
    ("negative window", dict(window=-5), E_INVALID, "window = -5"),
    ("window without causal", dict(window=8, causal=0), E_INVALID, "causal = 0"),
    ("window = 0 in a call with nothing to do", dict(window=0, batch=0), E_INVALID, "window"),
    ("window before the formats", dict(window=0, fmts=[WC._fmt(), WC._fmt(32), WC._fmt(), WC._fmt()]), E_INVALID, "window"),
    # the sibling's, which still apply
    ("D = 24", dict(window=8, D=24), E_UNSUPPORTED, "head dim"),
    ("P block 32", dict(window=8, fmts=[WC._fmt(), WC._fmt(), WC._fmt(32), WC._fmt()]), E_UNSUPPORTED, "quantizer"),
    ("null q", dict(window=8, q=None), E_INVALID, "null"),
    ("null workspace", dict(window=8, ws=None), E_INVALID, "null"),
    ("short workspace", dict(window=8, ws_bytes=WS_OK - 1), E_INVALID, "workspace"),
    ("workspace not 16-byte aligned", dict(window=8, ws=0x50008), E_INVALID, "aligned"),
    ("null block_table", dict(window=8, tbl=None), E_INVALID, "KV pool"),
    ("null lens", dict(window=8, lens=None), E_INVALID, "KV pool"),
    ("max_len > 16 table_stride", dict(window=8, max_len=65), E_INVALID, "KV pool"),
    ("short pool", dict(window=8, pool_bytes=1000), E_INVALID, "KV pool"),
])
def test_refusals_before_any_gpu_call(name, case, kwargs, want, word):
    rc, msg = _attend(name, **kwargs)
    assert rc == want, (case, rc, msg)
    assert name[5:] in msg and word in msg and len(msg) > 20, (case, msg)


def test_the_ragged_entry_keeps_its_siblings_own_refusals():
    for kwargs, word in ((dict(starts=None), "KV pool"), (dict(S=0), "max_s")):
        rc, msg = _attend("lqer_attention_q_paged_ragged_window", window=8, **kwargs)
        assert rc == E_INVALID and "attention_q_paged_ragged_window" in msg and word in msg, msg


@pytest.mark.parametrize("name", list(PAIRS))
def test_a_short_workspace_names_the_size_function_that_exists(name):
    rc, msg = _attend(name, window=8, ws_bytes=WS_OK - 1)
    assert rc == E_INVALID and f"(lqer_{PAIRS[name][5:]}_workspace_bytes)" in msg and f"< {WS_OK} B" in msg, msg


@pytest.mark.parametrize("name", list(PAIRS))
def test_nothing_to_do_is_ok_with_a_valid_window(name):
    assert _attend(name, window=8, batch=0, q=None, out=None, ws=None)[0] == 0
    assert _attend(name, window=1 << 62, batch=0)[0] == 0


# ---- PagedKVCache(max_query_rows=R) ---------------------------------------------------------------------------------------------------
def _host_cache(num_pages, max_seqs, window, max_pages_per_seq, rows, launch=None):
    """test_kv_window_cpu's host cache, made with max_query_rows (absent: the default constructor call)."""
    import json

    with open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")) as fh:
        cfg = json.load(fh)
    from lqer_amd.kvcache import PagedKVCache

    kw = {} if rows == "default" else {"max_query_rows": rows}
    cache = PagedKVCache(num_pages, max_seqs, 2, 16, cfg, cfg, torch.float16, "cpu", max_pages_per_seq=max_pages_per_seq, window=window, **kw)
    cache._launch_append = cache._launch_append_ragged = launch or (lambda *a: None)
    return cache


def test_max_query_rows_validation():
    for bad in (0, 7, -1, 8.0, 12.5, True, "12"):
        with pytest.raises(ValueError, match="max_query_rows"):
            _host_cache(4, 1, 16, 4, bad)
    for ok in (None, 8, 9, 512):
        assert _host_cache(4, 1, 16, 4, ok).max_query_rows == ok
        assert _host_cache(4, 1, None, 4, ok).max_query_rows == ok  # allowed without a window: nothing is ever released there
    assert _host_cache(4, 1, 16, 4, "default").max_query_rows is None


@pytest.mark.parametrize("R", [8, 12, 40])
@pytest.mark.parametrize("W", [4, 20, 33])
def test_the_release_rule_step_by_step(W, R):
    """released after every append is the rule's own arithmetic - and with R = 8 it is, step by step, what a cache made without the
    argument does on the same appends (append and append_ragged alike)."""
    rnd = random.Random(100 * W + R)
    cache, plain = _host_cache(64, 2, W, 160, R), _host_cache(64, 2, W, 160, "default")
    for c in (cache, plain):
        c.alloc(), c.alloc()
    t = [0, 0]
    gone = [0, 0]
    for step in range(60):
        if step % 2:
            counts = [rnd.randint(0, R), rnd.randint(1, R)]
            for c in (cache, plain):
                c.append_ragged([0, 1], torch.zeros(sum(counts), 2, 16, dtype=torch.float16), torch.zeros(sum(counts), 2, 16, dtype=torch.float16), counts)
        else:
            counts = [rnd.choice((1, R, rnd.randint(1, R)))] * 2
            for c in (cache, plain):
                c.append([0, 1], WC._kv(2, counts[0]), WC._kv(2, counts[0]))
        for b, n in enumerate(counts):
            if n:
                gone[b] = max(gone[b], min(t[b] + n - W - (R - 1), PAGE_KEYS * (t[b] // PAGE_KEYS)) // PAGE_KEYS, 0)
            t[b] += n
        assert cache.pt.released == gone and cache.pt.lengths == t, (step, counts)
        if R == 8:
            assert plain.pt.released == cache.pt.released and WC._books(plain.pt) == WC._books(cache.pt), step
        else:
            assert all(a <= b for a, b in zip(cache.pt.released, plain.pt.released))  # more rows to come: never more released
        WC._consistent(cache.pt)
    assert max(gone) > 0


@pytest.mark.parametrize("R", [8, 9, 12, 32, 40, 130, 512])
@pytest.mark.parametrize("W", [1, 4, 16, 20, 33, 70, 200])
def test_the_page_bound_is_held_and_reached_in_a_pool_of_its_size(W, R):
    """Appends of 1, R or a random count up to R keys to two sequences in a pool of exactly 2 ((W + R + 29) // 16) pages: never out
    of pages, the bound is reached, and every later call of s <= R rows still finds the page of its first row's first key."""
    bound = (W + R + 29) // 16
    rnd = random.Random(7 * W + R)
    cache = _host_cache(2 * bound, 2, W, max_pages_per_seq=1 << 12, rows=R)
    seqs = [cache.alloc(), cache.alloc()]
    most, t = 0, 0
    while t < 40 * (W + R):
        n = (1, R, rnd.randint(1, R))[rnd.randrange(3)] if t > 3 * (W + R) else 1
        cache.append(seqs, WC._kv(2, n), WC._kv(2, n))
        t += n
        for sq in seqs:
            gone = cache.pt.released[cache.pt.slot(sq)]
            assert cache.length(sq) == t and cache.pages_held(sq) <= bound
            for s in {1, 8, R, rnd.randint(1, R)}:
                assert PAGE_KEYS * gone <= max(0, t - s - W + 1), (t, s, gone)
        most = max(most, cache.pages_held(seqs[0]))
        WC._consistent(cache.pt)
    assert most == bound
    for sq in seqs:
        cache.free(sq)
    assert cache.pages_free == 2 * bound


def test_r_equal_8_is_the_documented_bound():
    assert all((W + 8 + 29) // 16 == (W + 37) // 16 for W in range(1, 300))


# ---- the Python refusals and the plan, on the host (nothing is launched: every refusal comes before the first device call) --------------
def _grown(W, R, n, step, **kw):
    cache = _host_cache(64, 4, W, 40, R, **kw)
    s = cache.alloc()
    for at in range(0, n, step):
        m = min(step, n - at)
        cache.append([s], WC._kv(1, m), WC._kv(1, m))
    return cache, s


def test_the_keys_are_gone_refusal():
    cache, s = _grown(20, 12, 100, 12)
    gone = cache.pt.released[0]
    assert gone == (100 - 20 - 11) // 16 == 4  # keys below 64 are gone
    # 17 rows start at key 100 - 17 - 20 + 1 = 64: still there - 18 rows reach key 63
    q = torch.zeros(1, 2, 18, 16, dtype=torch.float16)
    for kernel in ("prefill", "auto"):
        with pytest.raises(ValueError, match="released.*keys are gone"):
            attention_flexible_paged(q, cache, [s], 1.0, causal=True, kernel=kernel)
    qr = torch.zeros(18, 2, 16, dtype=torch.float16)
    for kernel in ("prefill", "auto"):
        with pytest.raises(ValueError, match="released.*keys are gone"):
            attention_flexible_paged_ragged(qr, cache, [s], [18], 1.0, causal=True, kernel=kernel)
    # the explicit W > cache.window refusal stays, in its own words
    with pytest.raises(ValueError, match="released the pages below the cache's window"):
        attention_flexible_paged(q[:, :, :12], cache, [s], 1.0, causal=True, kernel="prefill", window=21)
    with pytest.raises(ValueError, match="released the pages below the cache's window"):
        attention_flexible_paged_ragged(qr[:12], cache, [s], [12], 1.0, causal=True, kernel="prefill", window=21)


def test_a_default_cache_still_raises_the_two_old_errors():
    cache, s = _grown(20, "default", 100, 8)
    assert cache.max_query_rows is None and cache.pt.released[0] == (100 - 20 - 7) // 16
    q = torch.zeros(1, 2, 12, 16, dtype=torch.float16)
    for kernel in ("prefill", "auto"):
        with pytest.raises(ValueError, match="the prefill kernel has no window rule"):
            attention_flexible_paged(q, cache, [s], 1.0, causal=True, kernel=kernel)
        with pytest.raises(ValueError, match="the prefill kernel has no window rule"):
            attention_flexible_paged_ragged(q[0].transpose(0, 1), cache, [s], [12], 1.0, causal=True, kernel=kernel)
    plan = attention_flexible_paged_ragged.plan(cache, [s], [12])
    assert plan == [{"call": "lqer_attention_q_paged_ragged", "seqs": [0], "rows": "view", "window": None}]  # (no length is read: as ever)
    assert attention_flexible_paged_ragged.plan(cache, ["no such sequence"], [12]) == plan


def test_the_plan_names_the_window_of_the_prefill_call():
    cache, a = _grown(20, 40, 100, 40)
    b, c = cache.alloc(), cache.alloc()
    cache.append([b], WC._kv(1, 18), WC._kv(1, 18))
    cache.append([c], WC._kv(1, 5), WC._kv(1, 5))
    plan = attention_flexible_paged_ragged.plan
    assert plan(cache, [c, a, b], [1, 40, 12]) == [
        {"call": "lqer_attention_q_decode_paged_ragged", "seqs": [0], "rows": "view", "window": 20},
        {"call": "lqer_attention_q_paged_ragged_window", "seqs": [1, 2], "rows": "view", "window": 20}]
    assert plan(cache, [a, b], [40, 12], window=7)[0]["window"] == 7
    assert plan(cache, [a, c], [3, 2], kernel="prefill") == [
        {"call": "lqer_attention_q_paged_ragged_window", "seqs": [0, 1], "rows": "view", "window": 20}]
    # while every length the call addresses is <= W the unwindowed entry runs, as on any cache
    assert plan(cache, [c, b], [1, 12]) == [
        {"call": "lqer_attention_q_decode_paged_ragged", "seqs": [0], "rows": "view", "window": 20},
        {"call": "lqer_attention_q_paged_ragged", "seqs": [1], "rows": "view", "window": None}]
    with pytest.raises(ValueError):
        plan(cache, [a, 99], [40, 12])
    # a cache without a window: only an explicit window= switches the rule on
    free = _host_cache(16, 1, None, 8, 40)
    s = free.alloc()
    free.append([s], WC._kv(1, 60), WC._kv(1, 60))
    assert plan(free, [s], [12])[0] == {"call": "lqer_attention_q_paged_ragged", "seqs": [0], "rows": "view", "window": None}
    assert plan(free, [s], [12], window=30)[0] == {"call": "lqer_attention_q_paged_ragged_window", "seqs": [0], "rows": "view", "window": 30}
    assert free.pt.released == [0]

"""The refusals of the four attention entry points (lqer_attention_q, lqer_attention_q_decode, lqer_attention_q_decode_kv,
lqer_attention_q_kv), byte for byte: one table of cases, each applied to every call that has the case's argument, replayed against
the built library and compared - return code AND lqer_last_error() text - with tests/golden/attn_refusals.json, a recording of the
library before the four calls came to share one argument record and one check.  The pointers are made-up constants, so the %p texts
are reproducible; every case is refused, or has nothing to do, before anything touches a device.

`python tests/test_attention_refusals_cpu.py --record` rewrites the fixture from the built library (LQER_AMD_LIB names another build)."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # (run as a script: the package is found from the repository's root)
    sys.path.insert(0, ROOT)

from lqer_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_refusals.json")
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -2
PREFILL, DECODE = ("lqer_attention_q", "lqer_attention_q_kv"), ("lqer_attention_q_decode", "lqer_attention_q_decode_kv")
RAW, CACHED = ("lqer_attention_q", "lqer_attention_q_decode"), ("lqer_attention_q_kv", "lqer_attention_q_decode_kv")
CALLS = (PREFILL[0], DECODE[0], DECODE[1], PREFILL[1])
COMMON = {"q", "mask", "out", "dtype", "batch", "heads", "kv", "S", "T", "D", "q_strides", "mask_strides", "out_strides", "causal", "fmts", "ws",
          "ws_bytes"}
ARGS = {name: COMMON | ({"k", "v", "k_strides", "v_strides"} if name in RAW else {"cache", "cache_bytes", "capacity"}) for name in CALLS}
SHORT = "one byte short"  # ws_bytes / cache_bytes: what the call's own size function asks, less one


def _fmt(block=16, width=8, kind=_lib.Q_MXINT):
    return _lib.QFmt(kind, width, block, 8, 127)


MINIFLOAT = _lib.QFmt(_lib.Q_MINIFLOAT, 8, 16, 4, 7)
NO_DATA = dict(q=None, k=None, v=None, cache=None, mask=None, out=None, ws=None)

# (case, arguments, calls): the case runs on every call of `calls` (None: all four) that has its FIRST argument; arguments a call does
# not have are left out.  A valid call would reach the device: every case here is refused or has nothing to do.
CASES = [
    # ---- one fault: the union of test_attention_fused_cpu, test_attention_decode_cpu, test_kv_cache_cpu and test_kv_prefill_cpu
    ("null q", dict(q=None), None),
    ("null k", dict(k=None), None),
    ("null v", dict(v=None), None),
    ("null out", dict(out=None), None),
    ("null workspace", dict(ws=None), None),
    ("D = 24", dict(D=24), None),
    ("D = 144", dict(D=144), None),
    ("P block 32", dict(fmts=[_fmt(), _fmt(), _fmt(32), _fmt()]), None),
    ("V block 32", dict(fmts=[_fmt(), _fmt(), _fmt(), _fmt(32)]), None),
    ("Q width 12", dict(fmts=[_fmt(width=12), _fmt(), _fmt(), _fmt()]), None),
    ("K minifloat", dict(fmts=[_fmt(), MINIFLOAT, _fmt(), _fmt()]), None),
    ("null format", dict(fmts=[_fmt(), _fmt(), None, _fmt()]), None),
    ("null q strides", dict(q_strides=False), None),
    ("null k strides", dict(k_strides=False), None),
    ("null v strides", dict(v_strides=False), None),
    ("null out strides", dict(out_strides=False), None),
    ("null mask strides", dict(mask_strides=False, mask=0x60000), None),
    ("heads % kv_heads", dict(heads=6, kv=4), None),
    ("mask and causal", dict(mask=0x60000, causal=1), None),
    ("short workspace", dict(ws_bytes=SHORT), None),
    ("workspace not 16-byte aligned", dict(ws=0x50008), CALLS[1:]),  # (the raw prefill takes it: see the two-fault case)
    ("negative batch", dict(batch=-1), None),
    ("kv_heads = 0", dict(kv=0), None),
    ("negative S", dict(S=-1), None),
    ("negative T", dict(T=-1), None),
    ("T = 0", dict(T=0), None),
    ("unknown dtype", dict(dtype=9), None),
    ("S = 9", dict(S=9), DECODE),
    ("S = 9, short workspace", dict(S=9, ws_bytes=SHORT), None),
    ("S = 1000, short workspace", dict(S=1000, ws_bytes=SHORT), None),
    ("S = 1000, short cache", dict(cache_bytes=SHORT, S=1000), None),
    ("null cache", dict(cache=None), None),
    ("cache not 16-byte aligned", dict(cache=0x100008), None),
    ("short cache", dict(cache_bytes=SHORT), None),
    ("T > capacity", dict(capacity=64, T=65), None),  # (everything else valid: the cache's check)
    ("capacity = 0", dict(capacity=0), None),
    # ---- two faults: the order of the checks
    ("S = 9 and D = 24", dict(S=9, D=24), None),  # decode: S
    ("null format, mask and causal", dict(fmts=[_fmt(), None, _fmt(), _fmt()], mask=0x60000, causal=1), None),  # the mask
    ("D = 144 and block 32", dict(D=144, fmts=[_fmt(), _fmt(32), _fmt(), _fmt()]), None),  # D
    ("batch = 0, no data pointer", dict(batch=0, **NO_DATA), None),  # OK
    ("S = 0, no data pointer", dict(S=0, **NO_DATA), None),  # OK
    ("batch = 0 and T = 0", dict(batch=0, T=0), None),  # OK
    ("T = 0 and null q", dict(T=0, q=None), None),  # T
    ("short workspace and short cache", dict(cache_bytes=SHORT, ws_bytes=SHORT), None),  # the attention check speaks first
    ("workspace misaligned by 8 and short", dict(ws=0x50008, ws_bytes=SHORT), None),  # raw prefill: the size; the others: the alignment
    # ---- the launch grid of each kernel
    ("T beyond the image grid", dict(T=65535 * 64 + 1, capacity=1 << 23, cache_bytes=1 << 40, ws_bytes=1 << 40), PREFILL),
    ("batch x kv_heads beyond the grid", dict(batch=256, kv=256, heads=256, ws_bytes=1 << 40, cache_bytes=1 << 40), PREFILL),
    ("T beyond 2^30", dict(T=(1 << 30) + 1, capacity=1 << 31, cache_bytes=1 << 44, ws_bytes=1 << 44), None),
    ("kv_heads beyond the grid", dict(kv=65536, heads=65536, ws_bytes=1 << 40, cache_bytes=1 << 40), None),
]


def _table():
    """[(key, call, arguments)] of every case on every call it applies to."""
    out = []
    for case, kwargs, calls in CASES:
        for name in calls or CALLS:
            if next(iter(kwargs)) in ARGS[name]:
                out.append(("%s | %s" % (case, name), name, {k: v for k, v in kwargs.items() if k in ARGS[name]}))
    return out


def _call(name, q=0x10000, k=0x20000, v=0x30000, cache=0x100000, cache_bytes=1 << 24, capacity=64, mask=None, out=0x40000, ws=0x50000,
          ws_bytes=1 << 20, dtype=_lib.F16, batch=1, heads=4, kv=4, S=4, T=40, D=64, fmts=None, causal=0, q_strides=True, k_strides=True,
          v_strides=True, mask_strides=True, out_strides=True):
    L = _lib.lib()
    tri = lambda on, a, b, c: (C.c_int64 * 3)(a, b, c) if on else None
    fp = [C.byref(f) if f is not None else None for f in fmts or [_fmt()] * 4]
    if ws_bytes == SHORT:
        ws_bytes = getattr(L, name + "_workspace_bytes")(batch, heads, kv, S, T, D) - 1
    if cache_bytes == SHORT:
        cache_bytes = L.lqer_kv_cache_bytes(dtype, batch, kv, capacity, D) - 1
    qs, os_ = tri(q_strides, heads * S * D, S * D, D), tri(out_strides, heads * S * D, S * D, D)
    ms = tri(mask is not None and mask_strides, 0, 0, T)
    src = (k, v) if name in RAW else (cache, cache_bytes, capacity)
    kvs = (tri(k_strides, kv * T * D, T * D, D), tri(v_strides, kv * T * D, T * D, D)) if name in RAW else ()
    rc = getattr(L, name)(q, *src, mask, out, None, dtype, batch, heads, kv, S, T, D, qs, *kvs, ms, os_, 0.125, causal, *fp, ws, ws_bytes, None)
    return rc, L.lqer_last_error().decode()


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_table_is_the_recorded_one():
    assert sorted(key for key, _, _ in _table()) == sorted(_golden()["refusals"])
    assert len({key for key, _, _ in _table()}) == len(_table())


@pytest.mark.parametrize("key, name, kwargs", _table(), ids=[key for key, _, _ in _table()])
def test_refusal_is_the_recorded_one(key, name, kwargs):
    want_rc, want_msg = _golden()["refusals"][key]
    assert want_rc in (OK, E_INVALID, E_UNSUPPORTED), key  # (nothing recorded here got as far as a launch)
    before = _call(name, dtype=9)[1]  # a refusal first: a success leaves lqer_last_error() as it was
    rc, msg = _call(name, **kwargs)
    assert rc == want_rc, (key, rc, msg)
    assert msg == (want_msg if rc != OK else before), key


def test_the_order_of_the_checks():
    """What the two-fault cases are there to pin, read off the recording itself."""
    g = _golden()["refusals"]
    for name in CALLS:
        assert ("query rows" in g["S = 9 and D = 24 | " + name][1]) == (name in DECODE)
        assert "two forms of one mask" in g["null format, mask and causal | " + name][1]
        assert "head dim 144" in g["D = 144 and block 32 | " + name][1]
        assert g["batch = 0, no data pointer | " + name][0] == g["S = 0, no data pointer | " + name][0] == g["batch = 0 and T = 0 | " + name][0] == OK
        assert "T = 0" in g["T = 0 and null q | " + name][1]
        assert ("not 16-byte aligned" in g["workspace misaligned by 8 and short | " + name][1]) == (name != "lqer_attention_q")
        assert "beyond" in g["kv_heads beyond the grid | " + name][1] and g["T beyond 2^30 | " + name][0] == E_UNSUPPORTED
    assert " B < " in g["workspace misaligned by 8 and short | lqer_attention_q"][1]
    for name in CACHED:
        assert "workspace" in g["short workspace and short cache | " + name][1]
        assert "beyond the KV cache's capacity" in g["T > capacity | " + name][1]
    for name in PREFILL:
        assert "T = 4194241" in g["T beyond the image grid | " + name][1]
        assert "batch 256 x heads 256" in g["batch x kv_heads beyond the grid | " + name][1]
    for name in DECODE:
        assert "beyond 2^30 keys" in g["T beyond 2^30 | " + name][1] and "kv_heads 65536" in g["kv_heads beyond the grid | " + name][1]


def _record(commit):
    refusals = {}
    for key, name, kwargs in _table():
        rc, msg = _call(name, **kwargs)
        assert rc in (OK, E_INVALID, E_UNSUPPORTED), (key, rc, msg)  # anything else got as far as a launch: not a case for this table
        refusals[key] = [rc, msg if rc != OK else ""]
    with open(GOLDEN, "w") as fh:
        json.dump({"recorded_from": commit, "refusals": refusals}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %d refusals of %s into %s" % (len(refusals), _lib.LIB_PATH, GOLDEN))


if __name__ == "__main__":
    if "--record" not in sys.argv[1:]:
        sys.exit("usage: python tests/test_attention_refusals_cpu.py --record [COMMIT]")
    rest = [a for a in sys.argv[1:] if a != "--record"]
    _record(rest[0] if rest else "the working tree")

"""Time ONE decode attention call over beams forked from one parent with the shared prefix read once per group
(attention_flexible_paged(..., shared_prefix=True): lqer_attention_q_decode_paged_shared) against the same call as it was
(shared_prefix=False: lqer_attention_q_decode_paged, which this entry does not touch), in this process on the same pool, with HIP events.

    python tools/kv_paged_shared_bench.py [--steps 30] [--warmup 5] [--rounds 5] [--out profiles/kv_paged_shared.json]

The workload: a parent of `prefix` keys is forked into `width` beams and every beam is appended ONE key of its own, so the beams hold
16 (prefix // 16) keys on the same pages and an open block each; then one query row per head attends (s = 1, no mask).  Heads 32 / 32
(Llama-7B: one query row per kv head and beam) and 32 / 8 (grouped-query: four), d = 128, fp16; widths 4, 8 and 16; prefixes of 1029
and 4101 keys.  Two legs, alternating over several rounds with every round reported:
  shared    shared_prefix=True - the groups are built from the host's books and uploaded with the call's metadata, a shared chunk is
            loaded by its group's leader alone, which runs the rows of all beams;
  plain     shared_prefix=False - every beam's workgroups load every chunk.
`timed` and the buffer rotation are tools/attn_bench.py's; what is timed is a CALL as a user makes it, Python and launches included -
for the shared leg also the grouping of the call's sequences from the host's books and the upload of the groups.  `shared_launches` /
`plain_launches` time the library entry alone, its argument tuple built once per pool beforehand (lqer_amd.kvcache._paged_args): the three
launches without the Python around them.
Recorded next to the times, by construction (not measured): the K / V bytes - codes and block exponents, 2 D (1 + 1/16) per key and kv
head - that the workgroups of each leg load, and the workgroups per kernel (scores, pv) that do work instead of leaving at once.
No bar is set: the numbers are recorded.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attn_bench import L3_BYTES, timed  # noqa: E402
from lqer_amd import PagedKVCache, _lib, attention_flexible_paged, kvcache, ops  # noqa: E402

H, D = 32, 128
ENTRIES = [(hk, w, n) for hk in (32, 8) for n in (1029, 4101) for w in (4, 8, 16)]
LEGS = ("shared", "plain", "shared_launches", "plain_launches")


def by_construction(hk, width, t, shared_keys):
    """(K / V bytes loaded, workgroups per kernel that do work) of both legs for `width` sequences of t keys that share `shared_keys`."""
    C = _lib.lib().lqer_attention_q_decode_chunk(t, D)
    nch, n_shared = -(-t // C), shared_keys // C
    per_key = hk * 2 * (D + D // 16)
    plain = {"kv_bytes": width * t * per_key, "workgroups": width * hk * nch}
    shared = {"kv_bytes": (width * t - (width - 1) * n_shared * C) * per_key, "workgroups": hk * (n_shared + width * (nch - n_shared))}
    return {"chunk_keys": C, "chunks": nch, "shared_chunks": n_shared, "shared": shared, "plain": plain}


def one_entry(hk, width, n, cfg, a):
    dt, name = torch.float16, f"heads{H}_{hk}_width{width}_len{n}"
    stride = (n + 1 + 15) // 16
    pages = n // 16 + 2 * width
    make = lambda: PagedKVCache(pages, width + 1, hk, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)
    pool_bytes = make().nbytes
    nbuf = max(3, min(16, -(-3 * L3_BYTES // pool_bytes)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(hk + width + n)
    bufs = []
    for _ in range(nbuf):
        pool = make()
        first = pool.alloc()
        pool.append([first], *(torch.randn(1, hk, n, D, generator=g, device="cuda", dtype=dt) for _ in range(2)))
        beams = [first] + pool.fork(first, width - 1)
        pool.append(beams, *(torch.randn(width, hk, 1, D, generator=g, device="cuda", dtype=dt) for _ in range(2)))
        bufs.append((pool, beams, torch.randn(width, H, 1, D, generator=g, device="cuda", dtype=dt)))
    scaling = D ** -0.5
    pool, beams, _ = bufs[0]
    slots = pool.pt.slots(beams)
    groups = pool.pt.prefix_groups(slots, [n + 1] * width, lambda t: _lib.lib().lqer_attention_q_decode_chunk(t, D))
    assert groups == [(list(range(width)), 16 * (n // 16))], groups

    # the entries alone: one argument tuple per pool and leg, the metadata - the same for both legs - uploaded once
    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    ws = ops.workspace(dev, L.lqer_attention_q_decode_paged_workspace_bytes(width, H, hk, 1, pool.pt.max_len, D))
    out = torch.empty(width, H, 1, D, device="cuda", dtype=dt)
    built = {}
    for pool_i, beams_i, q_i in bufs:
        sl = pool_i.pt.slots(beams_i)
        built[id(pool_i)] = {leg: kvcache._paged_args(kvcache.PAGED_DECODE, q_i, out, None, pool_i, sl, [n + 1] * width, scaling, False, None, ws.data_ptr(),
                                                      ws.numel(), ops._stream(dev), S=1, groups=groups if leg == "shared" else None)
                             for leg in ("shared", "plain")}
    assert built[id(pool)]["shared"][0] == kvcache.SHARED_DECODE and built[id(pool)]["plain"][0] == kvcache.PAGED_DECODE

    def launches(leg):
        def fn(pool, beams, q):
            name, args = built[id(pool)][leg]
            _lib.check(getattr(L, name)(*args), name)
        return fn

    fns = {"shared": lambda pool, beams, q: attention_flexible_paged(q, pool, beams, scaling, out_layout="bshd", shared_prefix=True),
           "plain": lambda pool, beams, q: attention_flexible_paged(q, pool, beams, scaling, out_layout="bshd"),
           "shared_launches": launches("shared"), "plain_launches": launches("plain")}
    same = bool(torch.equal(fns["shared"](*bufs[0]), fns["plain"](*bufs[0])))
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    res = {"entry": name, "heads": [H, hk], "d": D, "dtype": "float16", "width": width, "prefix_keys": n, "keys_per_beam": n + 1,
           "shared_keys": groups[0][1], "buffers": nbuf, "pool_bytes": pool_bytes, "same_bits": same}
    res.update(by_construction(hk, width, n + 1, groups[0][1]))
    for leg in LEGS:
        res[f"us_{leg}"] = round(med[leg], 1)
        res[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    res["plain_rounds_spread_frac"] = round((max(rounds["plain"]) - min(rounds["plain"])) / med["plain"], 4)
    res["shared_over_plain"] = round(med["shared"] / med["plain"], 4)
    res["shared_launches_over_plain_launches"] = round(med["shared_launches"] / med["plain_launches"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_shared.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_shared_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    with torch.no_grad():
        entries = [one_entry(hk, w, n, cfg, a) for hk, w, n in ENTRIES]
    out = {"tool": "tools/kv_paged_shared_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call included (shared: the groups built from the host's "
           "books and one more small upload; *_launches: the library entry alone on an argument tuple built beforehand); one decode attention call, one query row per head, over `width` beams forked from one parent "
           "of `prefix_keys` keys with one own key each; kv_bytes and workgroups by construction, per leg", "entries": entries}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not all(e["same_bits"] for e in entries):
        raise SystemExit("the call with shared_prefix=True differs from the call without")


if __name__ == "__main__":
    main()

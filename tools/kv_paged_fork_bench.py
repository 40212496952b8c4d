"""Time a beam step over the paged KV pool with forked sequences (lqer_amd.kvcache.PagedKVCache.reorder: lqer_kv_pool_fork) against the
only route to a second sequence with the same prefix there was before it - alloc plus an append of the whole prefix from raw K and V -
in this process on the same box, with HIP events.

    python tools/kv_paged_fork_bench.py [--steps 30] [--warmup 5] [--rounds 5] [--out profiles/kv_paged_fork.json]

A step: every beam of the next step continues ONE parent (reorder(beams, [0] * width) - the worst case: width - 1 sequences are
dropped and width - 1 are made), then one new key per beam is appended, then the decode attention of one query row per head runs over
the beams.  Llama-7B's kv heads (32 / 32, d = 128), fp16; widths 4 and 8; prefixes of 1029 and 4101 keys (an open block of 5 keys: the
fork copies an item per child).  Two legs on the same values, alternating over several rounds with every round reported:
  fork      reorder() - the dropped beams' pages go back, the children share the parent's full pages, one launch copies the open
            block's item and the staging rows per child;
  rebuild   free() the dropped beams, alloc() as many, and ONE append of the prefix's raw K and V for all of them (the caller would
            have had to keep those tensors, which is what the cache exists to avoid), the rest of the step the same calls.
`reorder_only` / `rebuild_only` time the two first parts alone.  `timed` and the buffer rotation are tools/attn_bench.py's; what is timed
is a CALL as a user makes it, Python and launches included.  A timed step is repeated at one length: the host lengths are set back, and
the key a step appended is overwritten by the next (the staging rows below the prefix's length are never touched).
Bytes: the fork writes n kv_heads (34 D + 16 D esz) bytes for n children by construction - asserted here against the layout's spans and
against the bytes of the pool that a fork changes; the rebuild reads the raw prefix and writes every code and exponent of it, per child.
Pages in use with sharing against without are the allocator's counts.  No bar is set: the numbers are recorded.  Not part of bench.py.
Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attn_bench import L3_BYTES, timed  # noqa: E402
from lqer_amd import PagedKVCache, attention_flexible_paged  # noqa: E402

H, HK, D, ESZ = 32, 32, 128, 2
ENTRIES = [(w, n) for n in (1029, 4101) for w in (4, 8)]
LEGS = ("fork", "rebuild", "reorder_only", "rebuild_only")
up = lambda v: (v + 255) // 256 * 256


def fork_spans(pool, pages, slots):
    """Byte spans of the pool a fork may write for children with these tail pages and slots (include/lqer_hip.h's layout)."""
    items = pool.num_pages * HK
    spans, at = [], 0
    for per_item in (16 * D, D, 16 * D, D):
        spans += [(at + p * HK * per_item, at + (p + 1) * HK * per_item) for p in pages]
        at += up(items * per_item)
    per_slot = HK * 16 * D * ESZ
    return spans + [(at + s * per_slot, at + (s + 1) * per_slot) for s in slots]


def check_fork_bytes(pool, beams, width):
    """The bytes one reorder(beams, [0] * width) changes lie in the children's tail items and staging rows, which are
    (width - 1) kv_heads (34 D + 16 D esz) bytes."""
    for s in beams[1:]:  # whatever the children will land on differs from the parent's bytes
        slot = pool.pt.slot(s)
        for lo, hi in fork_spans(pool, [pool.pt.table[slot][pool.pt.pages_of[slot] - 1]], [slot]):
            pool.buf[lo:hi] ^= 0xFF
    snap = pool.buf.clone()
    new = pool.reorder(beams, [0] * width)
    kids = [pool.pt.slot(s) for s in new[1:]]
    allowed = torch.zeros(pool.buf.numel(), dtype=torch.bool, device="cuda")
    for lo, hi in fork_spans(pool, [pool.pt.table[s][pool.pt.pages_of[s] - 1] for s in kids], kids):
        allowed[lo:hi] = True
    changed = pool.buf != snap
    want = (width - 1) * HK * (34 * D + 16 * D * ESZ)
    assert int(allowed.sum()) == want, (int(allowed.sum()), want)
    assert not bool((changed & ~allowed).any()) and bool(changed.any())
    return new, want


def one_entry(width, n, cfg, a):
    dt, name = torch.float16, f"width{width}_len{n}"
    assert n % 16  # an open block: the fork copies an item per child
    pages_shared, pages_apart = n // 16 + width, width * ((n + 15) // 16)
    stride = (n + 1 + 15) // 16
    make = lambda: PagedKVCache(pages_apart, width, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)  # (room for the rebuild leg)
    pool_bytes = make().nbytes
    nbuf = max(3, min(16, -(-3 * L3_BYTES // pool_bytes)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(width + n)
    bufs, fork_bytes = [], None
    for i in range(nbuf):
        q = torch.randn(width, H, 1, D, generator=g, device="cuda", dtype=dt)
        k, v = (torch.randn(1, HK, n, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
        kn, vn = (torch.randn(width, HK, 1, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
        states = []
        for _ in range(2):  # one pool per leg family: the fork's, the rebuild's
            pool = make()
            first = pool.alloc()
            pool.append([first], k, v)
            st = types.SimpleNamespace(pool=pool, beams=[first] + pool.fork(first, width - 1), q=q, k=k, v=v, kn=kn, vn=vn)
            states.append(st)
        if i == 0:
            assert states[0].pool.pages_free == pages_apart - pages_shared and states[0].pool.pages_shared == n // 16
            states[0].beams, fork_bytes = check_fork_bytes(states[0].pool, states[0].beams, width)
        bufs.append(tuple(states))
    scaling = D ** -0.5

    def set_back(st):
        for s in st.beams:
            st.pool.pt.lengths[st.pool.pt.slot(s)] = n

    def reorder_only(f, r):
        f.beams = f.pool.reorder(f.beams, [0] * width)

    def rebuild_only(f, r):
        for s in r.beams[1:]:
            r.pool.free(s)
        new = [r.pool.alloc() for _ in range(width - 1)]
        r.pool.append(new, r.k.expand(width - 1, HK, n, D), r.v.expand(width - 1, HK, n, D))
        r.beams = [r.beams[0]] + new

    def rest(st):
        st.pool.append(st.beams, st.kn, st.vn)
        return attention_flexible_paged(st.q, st.pool, st.beams, scaling, out_layout="bshd")

    def fork_step(f, r):
        set_back(f)
        reorder_only(f, r)
        return rest(f)

    def rebuild_step(f, r):
        set_back(r)
        rebuild_only(f, r)
        return rest(r)

    fns = {"fork": fork_step, "rebuild": rebuild_step, "reorder_only": reorder_only, "rebuild_only": rebuild_only}
    same = bool(torch.equal(fork_step(*bufs[0]), rebuild_step(*bufs[0])))
    for f, r in bufs:
        set_back(f), set_back(r)
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            if leg.endswith("_only"):
                for f, r in bufs:
                    set_back(f), set_back(r)
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    kids, blocks = width - 1, (n + 15) // 16
    out = {"entry": name, "width": width, "prefix_keys": n, "kv_heads_d": [HK, D], "dtype": "float16", "buffers": nbuf, "same_bits": same,
           "children_per_step": kids, "pool_bytes": pool_bytes,
           "fork_bytes_written": fork_bytes, "fork_bytes_read": fork_bytes,
           "rebuild_bytes_read": kids * HK * n * D * ESZ * 2,  # raw K and V of the prefix
           "rebuild_bytes_written": kids * HK * (blocks * 17 * D + n * (D + D // 16) + (n % 16) * D * ESZ),  # K blocks whole, V rows, staging
           "pages_in_use_shared": pages_shared, "pages_in_use_apart": pages_apart}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    out["rebuild_rounds_spread_frac"] = round((max(rounds["rebuild"]) - min(rounds["rebuild"])) / med["rebuild"], 4)
    out["fork_over_rebuild"] = round(med["fork"] / med["rebuild"], 4)
    out["reorder_only_over_rebuild_only"] = round(med["reorder_only"] / med["rebuild_only"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_fork.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_fork_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    with torch.no_grad():
        entries = [one_entry(w, n, cfg, a) for w, n in ENTRIES]
    out = {"tool": "tools/kv_paged_fork_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call included; a step = every beam continues one "
           "parent (fork: reorder; rebuild: free + alloc + append of the prefix from raw K and V) + append of one key per beam + decode "
           "attention of one query row per head", "entries": entries}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not all(e["same_bits"] for e in entries):
        raise SystemExit("the step over forked sequences differs from the step over rebuilt ones")


if __name__ == "__main__":
    main()

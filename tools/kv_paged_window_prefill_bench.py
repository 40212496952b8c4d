"""Time a prompt CHUNK over the paged KV pool with a sliding window (lqer_amd.kvcache.PagedKVCache(window=W, max_query_rows=512):
lqer_kv_pool_append + lqer_attention_q_paged_window - k_attn_q's window rule on images written from the window's first tile on, old
pages released) against the same chunk on the same sequences with every page kept and window=None (lqer_attention_q_paged with the
causal rule - the only route there was for such a chunk before the prefill kernel had the rule), in this process on the same box,
with HIP events.

    python tools/kv_paged_window_prefill_bench.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/kv_paged_window_prefill.json]

A step is the append of 512 new keys per sequence plus the attention of their 512 query rows per head (kernel="prefill"), at
Llama-7B's heads (32 / 32, d = 128), fp16, batch 8, causal.  Histories of 4101 and 16389 keys after the chunk, windows of 1024 and 4096
keys: per history one unwindowed leg and one leg per window, alternating over several rounds with every round reported.  The method is
tools/kv_paged_window_bench.py's: `timed` and the buffer rotation are tools/attn_bench.py's (enough distinct pools per leg that the
Infinity Cache holds none of them, counted from the pages a leg's sequences hold); what is timed is a CALL as a user makes it, Python
and launches included.  The timed step is repeated at one length: the host lengths are set back, the append rewrites the same blocks
from the staging rows and the same new keys, and a windowed sequence has nothing more to release.  A pool is built up to the chunk and
its FIRST step is the genuine append - the one whose bits are checked; from the second on the staging rows hold the chunk's last
keys instead of the history's (the chunk starts inside a block), so the open block's codes differ - the work does not.
The windowed sequences are grown in appends of up to 512 keys, releasing on the way, in a pool of exactly the bound
(W + 512 + 29) // 16 pages per sequence; both legs' tables have room for the whole history.
Per entry: microseconds per leg (median of the rounds) and every round, the spread of the unwindowed leg's rounds, the ratio of the
medians, the pages in use per leg, and whether the windowed output of the first sequence is, bit for bit, the prefill kernel's on the
full raw K and V with the window as a mask tensor.  No bar is set: the numbers are recorded (the expectation from the code is work per
chunk that follows W + 512 instead of the history).  Not part of bench.py.  Needs a GPU: there is no fall-back."""
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
from lqer_amd import PagedKVCache, attention_flexible, attention_flexible_paged  # noqa: E402

H, HK, D, B, CHUNK = 32, 32, 128, 8, 512
HISTORIES, WINDOWS = (4101, 16389), (1024, 4096)
PAGE_BYTES = HK * (2 * 16 * D + 2 * D)  # codes and exponents of K and V of one page, all kv heads


def _rotation(pages_touched):
    return max(3, min(64, -(-3 * L3_BYTES // (pages_touched * PAGE_BYTES))))  # the rotation spans three times the Infinity Cache


def _pool(t, w, k, v, cfg):
    """A pool holding the first t - CHUNK keys of k / v [B, HK, t, D] for B sequences, with window w (None: every page kept), set up
    so that the timed step - the append of the last CHUNK keys - can be repeated: (cache, seqs, the chunk's k and v, the host
    lengths to start from)."""
    per_seq = (t + 15) // 16
    if w is None:
        cache = PagedKVCache(B * per_seq, B, HK, D, cfg, cfg, torch.float16, "cuda", max_pages_per_seq=per_seq)
    else:
        cache = PagedKVCache(B * ((w + CHUNK + 29) // 16), B, HK, D, cfg, cfg, torch.float16, "cuda", max_pages_per_seq=per_seq, window=w,
                             max_query_rows=CHUNK)
    seqs = [cache.alloc() for _ in range(B)]
    at = 0
    while at < t - CHUNK:
        n = (t - at) % CHUNK or CHUNK  # the odd piece first: the timed chunk is a whole one
        cache.append(seqs, k[:, :, at:at + n], v[:, :, at:at + n])
        at += n
    new = (k[:, :, t - CHUNK:].clone(), v[:, :, t - CHUNK:].clone())
    past = {cache.pt.slot(s): t - CHUNK for s in seqs}
    return cache, seqs, new, past


def one_history(t, cfg, a):
    dt, scaling = torch.float16, D ** -0.5
    g = torch.Generator(device="cuda").manual_seed(t)
    k, v = (torch.randn(B, HK, t, D, generator=g, device="cuda", dtype=dt) for _ in range(2))  # one history for every buffer: the pools differ, not the values
    legs = {"full": None, **{f"w{w}": w for w in WINDOWS}}

    def step(q, cache, seqs, new, past):
        for slot, n in past.items():
            cache.pt.lengths[slot] = n
        cache.append(seqs, *new)
        return attention_flexible_paged(q, cache, seqs, scaling, causal=True, out_layout="bshd", kernel="prefill")  # (window: the cache's)

    def buffer(w):  # a pool, its queries and its first - genuine - step: (the buffer, that step's output for the first sequence)
        buf = (torch.randn(B, H, CHUNK, D, generator=g, device="cuda", dtype=dt), *_pool(t, w, k, v, cfg))
        return buf, step(*buf)[:1].clone()

    bufs, pages, first_out = {}, {}, {}
    for leg, w in legs.items():
        first, first_out[leg] = buffer(w)
        pages[leg] = sum(first[1].pages_held(s) for s in first[2])
        bufs[leg] = [first] + [buffer(w)[0] for _ in range(_rotation(pages[leg]) - 1)]

    same = {}
    for leg, w in legs.items():
        if w is None:
            continue
        q, got = bufs[leg][0][0], first_out[leg]
        p = torch.arange(CHUNK, device="cuda").view(CHUNK, 1) + (t - CHUNK)
        j = torch.arange(t, device="cuda").view(1, t)
        mask = torch.zeros(1, 1, CHUNK, t, device="cuda", dtype=dt).masked_fill_(~((j <= p) & (j > p - w))[None, None], torch.finfo(dt).min)
        want = attention_flexible(q[:1], k[:1], v[:1], cfg, cfg, scaling, attention_mask=mask, kernel="prefill", out_layout="bshd")
        same[leg] = bool(torch.equal(got, want))
        del mask, want
    del k, v
    rounds = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg in legs:
            rounds[leg].append(timed(step, bufs[leg], a.steps, a.warmup))
    med = {leg: statistics.median(x) for leg, x in rounds.items()}
    out = []
    for leg, w in legs.items():
        if w is None:
            continue
        out.append({"entry": f"t{t}_w{w}", "keys": t, "window": w, "chunk_rows": CHUNK, "batch": B, "heads_kvheads_d": [H, HK, D], "dtype": "float16",
                    "buffers_full": len(bufs["full"]), "buffers_window": len(bufs[leg]),
                    "pages_in_use_full": pages["full"], "pages_in_use_window": pages[leg], "page_bytes": PAGE_BYTES,
                    "pages_per_sequence_bound": (w + CHUNK + 29) // 16, "same_bits_as_mask_tensor_route": same[leg],
                    "us_full": round(med["full"], 1), "us_full_rounds": [round(x, 1) for x in rounds["full"]],
                    "us_window": round(med[leg], 1), "us_window_rounds": [round(x, 1) for x in rounds[leg]],
                    "full_rounds_spread_frac": round((max(rounds["full"]) - min(rounds["full"])) / med["full"], 4),
                    "window_over_full": round(med[leg] / med["full"], 4),
                    "keys_ratio_window_plus_chunk_over_history": round((w + CHUNK) / t, 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_window_prefill.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_window_prefill_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    entries = []
    with torch.no_grad():
        for t in HISTORIES:
            entries += one_history(t, cfg, a)
            torch.cuda.empty_cache()
    out = {"tool": "tools/kv_paged_window_prefill_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": ["full (window=None, every page kept, lqer_attention_q_paged)",
                    "window (PagedKVCache(window=W, max_query_rows=512), old pages released, lqer_attention_q_paged_window)"],
           "timing": "eager calls between HIP events: host side of a call included; a step = append of 512 keys per sequence + causal attention "
           "of their 512 query rows per head", "entries": entries}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if any(e["same_bits_as_mask_tensor_route"] is False for e in entries):
        raise SystemExit("the windowed chunk's output differs from the mask-tensor route's")


if __name__ == "__main__":
    main()

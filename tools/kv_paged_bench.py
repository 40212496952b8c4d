"""Time a decode step over the paged KV pool (lqer_amd.kvcache.PagedKVCache: lqer_kv_pool_append + lqer_attention_q_decode_paged) against
the same step over the dense packed cache (QuantizedKVCache: lqer_kv_cache_append + lqer_attention_q_decode_kv), in this process on the
same box, with HIP events.

    python tools/kv_paged_bench.py [--steps 100] [--warmup 10] [--rounds 5] [--out profiles/kv_paged.json]

A step is the append of one new key per sequence plus the attention of one query row per head, at Llama-7B's heads (32 / 32, d = 128),
fp16, batch 8.  Two entries, the legs on the same values, alternating over several rounds with every round reported:
 (a) uniform  all eight sequences at 2048 keys: paged against dense.  The two do the same arithmetic on the same codes (the outputs are
              compared: the same bits), so the difference is the price of the table - a page index in front of every block's loads,
              the lengths read from the device, the host's three small copies of metadata.
 (b) ragged   lengths (64, 128, 256, 512, 1024, 1536, 2048, 2048): paged against today's way, a dense cache of capacity 2048 for
              every sequence and an additive mask tensor over the padding.
`timed` and the buffer rotation are tools/attn_bench.py's (enough distinct caches that the Infinity Cache holds none of them); what is
timed is a CALL as a user makes it, Python and launches included.  The timed step is repeated at one length: the new key is the last
one of its block, so the dense append can be issued again (include/lqer_hip.h), and the paged side's host lengths are set back.
Per entry: microseconds per leg (median of the rounds) and every round, the spread of the dense leg's rounds, the ratio of the
medians, and the bytes of both caches (derivable from the header's layouts; tests/test_kv_paged_cpu.py asserts the arithmetic).
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
from lqer_amd import PagedKVCache, QuantizedKVCache, attention_flexible_cached, attention_flexible_paged  # noqa: E402

H, HK, D, CAP = 32, 32, 128, 2048
ENTRIES = [("uniform_8x2048", (2048,) * 8), ("ragged_64_to_2048", (64, 128, 256, 512, 1024, 1536, 2048, 2048))]
LEGS = ("dense", "paged")


def one_entry(name, lens, cfg, a):
    dt, b = torch.float16, len(lens)
    pages = sum((n + 15) // 16 for n in lens)
    uniform = len(set(lens)) == 1
    dense_bytes = QuantizedKVCache(b, HK, D, cfg, cfg, dt, "cuda", capacity=CAP).nbytes
    paged_bytes = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=CAP // 16).nbytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // min(dense_bytes, paged_bytes))))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(len(name))
    mask = None
    if not uniform:  # the padding of the dense leg: keys at and beyond a sequence's length
        j = torch.arange(CAP, device="cuda")[None, :]
        mask = torch.zeros(b, CAP, device="cuda", dtype=dt).masked_fill_(j >= torch.tensor(lens, device="cuda")[:, None], torch.finfo(dt).min)
        mask = mask[:, None, None, :]
    bufs = []
    for _ in range(nbuf):
        q = torch.randn(b, H, 1, D, generator=g, device="cuda", dtype=dt)
        k, v = (torch.randn(b, HK, CAP, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
        dense = QuantizedKVCache(b, HK, D, cfg, cfg, dt, "cuda", capacity=CAP)
        dense.append(k, v)
        paged = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=CAP // 16)
        seqs = [paged.alloc() for _ in lens]
        for i, n in enumerate(lens):
            paged.append([seqs[i]], k[i:i + 1, :, :n], v[i:i + 1, :, :n])
        # the step's new key per sequence: its last one (the dense leg's sequences all end at CAP)
        new_d = (k[:, :, CAP - 1:].clone(), v[:, :, CAP - 1:].clone())
        new_p = tuple(torch.stack([x[i, :, n - 1:n] for i, n in enumerate(lens)]) for x in (k, v))
        slots = [paged.pt.slot(s) for s in seqs]
        past = {s: n - 1 for s, n in zip(slots, lens)}  # the host lengths the timed step starts from
        bufs.append((q, dense, new_d, paged, seqs, new_p, past))
        del k, v
    scaling = D ** -0.5
    assert all(n % 16 == 0 for n in lens)  # (the new key closes its block: such an append can be repeated at the same length)

    def dense_step(q, dense, new_d, paged, seqs, new_p, past):
        dense.length = CAP - 1
        dense.append(*new_d)
        return attention_flexible_cached(q, dense, scaling, attention_mask=mask, out_layout="bshd")

    def paged_step(q, dense, new_d, paged, seqs, new_p, past):
        for slot, n in past.items():
            paged.pt.lengths[slot] = n
        paged.append(seqs, *new_p)
        return attention_flexible_paged(q, paged, seqs, scaling, out_layout="bshd")

    fns = {"dense": dense_step, "paged": paged_step}
    same = bool(torch.equal(dense_step(*bufs[0]), paged_step(*bufs[0]))) if uniform else None
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    out = {"entry": name, "lengths": list(lens), "heads_kvheads_d": [H, HK, D], "dtype": "float16", "buffers": nbuf,
           "dense_leg": "QuantizedKVCache of capacity 2048" + ("" if uniform else " + additive mask tensor over the padding"),
           "same_bits": same, "pages": pages, "dense_cache_bytes": dense_bytes, "paged_pool_bytes": paged_bytes,
           "pool_over_dense_bytes": round(paged_bytes / dense_bytes, 4)}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    out["dense_rounds_spread_frac"] = round((max(rounds["dense"]) - min(rounds["dense"])) / med["dense"], 4)
    out["paged_over_dense"] = round(med["paged"] / med["dense"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    with torch.no_grad():
        entries = [one_entry(name, lens, cfg, a) for name, lens in ENTRIES]
    out = {"tool": "tools/kv_paged_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call included; a step = append of one key per sequence + "
           "attention of one query row per head", "entries": entries}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if any(e["same_bits"] is False for e in entries):
        raise SystemExit("the paged step's output differs from the dense step's at uniform lengths")


if __name__ == "__main__":
    main()

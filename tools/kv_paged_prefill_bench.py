"""Time a chunk of a prompt attending over the paged KV pool with the prefill kernel - ONE attention_flexible_paged(kernel="prefill") over
the batch (lqer_attention_q_paged: the two bf16 images written from the pool through the block table, k_attn_q with per-sequence
lengths) - against the route the pool offered before it: per sequence, to_dense(seq) (an allocation and a byte copy of the whole
sequence) and attention_flexible_cached(kernel="prefill") on the copy.  Both in this process on the same box, with HIP events.

    python tools/kv_paged_prefill_bench.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/kv_paged_prefill.json]

Shapes (fp16, Llama-7B's heads 32 / 32, d = 128, causal: the s queries are the last s tokens of every sequence):
    batch 4, s = 128, all lengths 2048;   batch 8, s = 64, the ragged lengths of kv_paged_bench.py (64 ... 2048);
    batch 1, s = 512, length 4096;        batch 1, s = 16, length 4096.
The method is tools/kv_paged_bench.py's: the legs alternate over several rounds and every round is reported; `timed` and the buffer
rotation are tools/attn_bench.py's (enough distinct pools that the Infinity Cache holds none of them); what is timed is a CALL as a
user makes it, Python, allocations and launches included.  Per shape: microseconds per leg (median of the rounds) and every round,
the parent leg's spread, the ratio, whether every sequence's output is the same bits on both legs, and the bytes each leg needs
beside the pool - the dense copies (and the image workspace of the longest one) against the image workspace of the batch.
The criterion: at the two batched shapes the paged leg's MEDIAN lies below the parent leg's FASTEST SINGLE ROUND (the rule of
tools/kv_cache_bench.py: both legs run the same attention kernel, the difference is the launches, copies and allocations removed, so
the margin is the parent's own spread).  The batch-1 shapes are reported without a gate: there the attention kernel is nearly all of
the call and the saving is the gather and the allocation.  `criterion_met` says so per gated shape; the tool exits non-zero when it
does not hold or when outputs differ.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
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
from kv_paged_bench import ENTRIES  # noqa: E402
from lqer_amd import PagedKVCache, QuantizedKVCache, _lib, attention_flexible_cached, attention_flexible_paged  # noqa: E402

H, HK, D = 32, 32, 128
SHAPES = [("batch4_s128_t2048", 128, (2048,) * 4, True), ("batch8_s64_ragged_64_to_2048", 64, dict(ENTRIES)["ragged_64_to_2048"], True),
          ("batch1_s512_t4096", 512, (4096,), False), ("batch1_s16_t4096", 16, (4096,), False)]  # name, s, lengths, gated
LEGS = ("parent", "paged")


def one_shape(name, s, lens, gated, cfg, a):
    dt, b = torch.float16, len(lens)
    pages = sum((n + 15) // 16 for n in lens)
    stride = (max(lens) + 15) // 16
    pool_bytes = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride).nbytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // (pool_bytes + b * H * s * D * 2))))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda").manual_seed(len(name) + s)
    bufs = []
    for _ in range(nbuf):
        q = torch.randn(b, H, s, D, generator=g, device="cuda", dtype=dt)
        paged = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)
        seqs = [paged.alloc() for _ in lens]
        for sq, n in zip(seqs, lens):
            k, v = (torch.randn(1, HK, n, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
            paged.append([sq], k, v)
            del k, v
        bufs.append((q, paged, seqs))
    scaling = D ** -0.5

    def parent(q, paged, seqs):  # what the pool offered for more than 8 query rows: one sequence at a time
        return [attention_flexible_cached(q[i:i + 1], paged.to_dense(sq), scaling, causal=True, out_layout="bshd", kernel="prefill")
                for i, sq in enumerate(seqs)]

    def paged_call(q, paged, seqs):
        return attention_flexible_paged(q, paged, seqs, scaling, causal=True, out_layout="bshd", kernel="prefill")

    fns = {"parent": parent, "paged": paged_call}
    want, got = parent(*bufs[0]), paged_call(*bufs[0])
    same = [bool(torch.equal(w, got[i:i + 1])) for i, w in enumerate(want)]
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    L = _lib.lib()
    max_len = min((max(lens) + 127) // 128 * 128, 16 * stride)  # what attention_flexible_paged hands the library
    out = {"shape": name, "batch": b, "s": s, "lengths": list(lens), "heads_kvheads_d": [H, HK, D], "dtype": "float16", "mask": "causal",
           "buffers": nbuf, "gated": gated, "same_bits": same, "pool_bytes": pool_bytes,
           "parent_dense_copy_bytes": sum(QuantizedKVCache(1, HK, D, cfg, cfg, dt, "cuda", capacity=max(n, 16)).nbytes for n in lens),
           "parent_workspace_bytes": max(L.lqer_attention_q_kv_workspace_bytes(1, H, HK, s, n, D) for n in lens),
           "paged_workspace_bytes": L.lqer_attention_q_paged_workspace_bytes(b, H, HK, s, max_len, D),
           "parent_launches": 4 * b, "paged_launches": 3}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    out["parent_rounds_spread_frac"] = round((max(rounds["parent"]) - min(rounds["parent"])) / med["parent"], 4)
    out["paged_over_parent"] = round(med["paged"] / med["parent"], 4)
    out["criterion_met"] = bool(med["paged"] < min(rounds["parent"])) if gated else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_prefill.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_prefill_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    shapes = []
    with torch.no_grad():
        for sh in SHAPES:
            shapes.append(one_shape(*sh, cfg, a))
            torch.cuda.empty_cache()
    ok = all(x["criterion_met"] for x in shapes if x["gated"]) and all(all(x["same_bits"]) for x in shapes)
    out = {"tool": "tools/kv_paged_prefill_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call (Python, allocations, launches) included",
           "criterion": "at the two batched shapes the paged leg's median below the fastest single round of the parent leg (per sequence "
                        "to_dense + attention_flexible_cached(kernel='prefill')); every sequence's output the same bits on both legs at every shape",
           "criterion_met": ok, "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the paged leg does not meet the criterion at a gated shape (or an output differs from the parent leg's)")


if __name__ == "__main__":
    main()

"""Time swapping a batch of sequences out of the paged KV pool to the host and back in (lqer_amd.kvcache.PagedKVCache.swap_out /
swap_in: lqer_kv_pool_copy) against the only route out of the pool there was before it - per sequence to_dense() + .cpu() - in this
process on the same box.

    python tools/kv_paged_swap_bench.py [--steps 10] [--warmup 2] [--rounds 3] [--out profiles/kv_paged_swap.json]

Batch 8 at 4101 and 16389 keys per sequence (an open block of 5 keys), 32 kv heads, d = 128, fp16; K and V block_fp of width 4 with a
byte per code and (code_bits=4) as nibbles.  Legs, alternating over several rounds with every round reported:
  swap_out   swap_out(seqs): one small upload of the id lists, ONE lqer_kv_pool_copy into a device image, one non-blocking copy into
             pinned host memory, the frees - timed up to image.synchronize();
  swap_in    swap_in(image): one copy of the host image up, the table rows and id lists up, ONE lqer_kv_pool_copy into the pool - timed
             up to the stream's end;
  to_dense   for every sequence to_dense(seq).buf.cpu(): a gather launch and a synchronous copy into pageable memory each.
ONLY THE OUTWARD LEG IS COMPARABLE: there was no way back into a pool, so swap_in has no counterpart here; and to_dense widens nibbles
to bytes and pads every sequence to a dense cache, so on the nibble pool it moves more bytes for the same keys.  Per leg: ms, launches
of the library per call (counted from the route), bytes that cross the host link, GB/s of those bytes.  What is timed is a CALL as a
user makes it - Python, allocation of the pinned buffer and launches included - with wall-clock time around a synchronize, since the legs
end on the host.  A round trip is checked to give the same decode attention bits as before it.  No bar is set: the link rate of the
machine is not a number of this project's, so the file records what was measured and against what.  Not part of bench.py.  Needs a
GPU: there is no fall-back."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lqer_amd import PagedKVCache, attention_flexible_paged  # noqa: E402

B, H, HK, D = 8, 32, 32, 128
LENS = (4101, 16389)
LEGS = ("swap_out", "swap_in", "to_dense")


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def one_entry(t, bits, cfg, a):
    dt, per_seq = torch.float16, (t + 15) // 16
    cache = PagedKVCache(B * per_seq, B, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=per_seq, code_bits=bits)
    g = torch.Generator(device="cuda").manual_seed(t)
    st = {"seqs": [cache.alloc() for _ in range(B)], "image": None}
    for at in range(0, t, 1024):  # (chunks: the raw K and V of the whole batch at once would be several GB)
        n = min(1024, t - at)
        k, v = (torch.randn(B, HK, n, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
        cache.append(st["seqs"], k, v)
    q = torch.randn(B, H, 1, D, generator=g, device="cuda", dtype=dt)
    want = attention_flexible_paged(q, cache, st["seqs"], D ** -0.5)

    def swap_out():
        st["image"] = cache.swap_out(st["seqs"])
        st["image"].synchronize()

    def swap_in():
        st["seqs"] = cache.swap_in(st["image"])

    def to_dense():
        return [cache.to_dense(s).buf.cpu() for s in st["seqs"]]

    dense_bytes = sum(x.numel() for x in to_dense())
    swap_out()
    image_bytes = st["image"].nbytes
    swap_in()
    same = bool(torch.equal(attention_flexible_paged(q, cache, st["seqs"], D ** -0.5), want))
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        outs, ins = [], []
        for i in range(a.warmup + a.steps):  # out and in alternate by nature: each is timed on its own, around a synchronize
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            swap_out()
            t1 = time.perf_counter()
            swap_in()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= a.warmup:
                outs.append((t1 - t0) * 1e3), ins.append((t2 - t1) * 1e3)
        rounds["swap_out"].append(statistics.mean(outs)), rounds["swap_in"].append(statistics.mean(ins))
        rounds["to_dense"].append(wall_ms(to_dense, a.steps, a.warmup))
    same = same and bool(torch.equal(attention_flexible_paged(q, cache, st["seqs"], D ** -0.5), want))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    moved = {"swap_out": image_bytes, "swap_in": image_bytes, "to_dense": dense_bytes}
    out = {"entry": f"t{t}_{'nibble' if bits else 'byte'}", "keys": t, "batch": B, "kv_heads_d": [HK, D], "dtype": "float16", "kv_width": 4,
           "code_bits": bits or 8, "pool_bytes": cache.nbytes, "same_bits_after_round_trips": same,
           "launches": {"swap_out": 1, "swap_in": 1, "to_dense": B}, "host_copies": {"swap_out": 1, "swap_in": 1, "to_dense": B}}
    for leg in LEGS:
        out[f"ms_{leg}"] = round(med[leg], 3)
        out[f"ms_{leg}_rounds"] = [round(x, 3) for x in rounds[leg]]
        out[f"bytes_{leg}"] = moved[leg]
        out[f"gbps_{leg}"] = round(moved[leg] / med[leg] / 1e6, 2)
    out["swap_out_over_to_dense"] = round(med["swap_out"] / med["to_dense"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_swap.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_swap_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    cfg["w_quantizer"] = dict(copy.deepcopy(cfg["w_quantizer"]), width=4)  # K (of Q K^T) and V (of P V): width 4; Q and P stay 8-bit
    entries = []
    with torch.no_grad():
        for t in LENS:
            for bits in (None, 4):
                entries.append(one_entry(t, bits, cfg, a))
                torch.cuda.empty_cache()
    out = {"tool": "tools/kv_paged_swap_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "compared_against": "per-sequence to_dense() + .cpu(), the only route out of the pool before lqer_kv_pool_copy; only "
           "the outward leg (swap_out) is comparable - nothing went into a pool before, so swap_in stands alone - and to_dense moves byte codes "
           "and dense padding, also from a nibble pool", "timing": "wall clock around whole calls, each ended by a synchronize: Python, the pinned "
           "allocation, the small uploads, the launch and the copy over the host link included; swap_out and swap_in alternate, each timed on "
           "its own", "threshold": None, "entries": entries}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not all(e["same_bits_after_round_trips"] for e in entries):
        raise SystemExit("a swapped sequence attends with other bits than before the swap")


if __name__ == "__main__":
    main()

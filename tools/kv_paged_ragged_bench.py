"""Time one MIXED scheduler step over the paged KV pool - most sequences decode one token while one or two arrivals take a prompt chunk -
done in one append_ragged plus one attention_flexible_paged_ragged(causal=True) (lqer_kv_pool_append_ragged; the decoders through
lqer_attention_q_decode_paged_ragged, the chunks through lqer_attention_q_paged_ragged) against the same step done the way the pool offered
before per-sequence counts, on the same commit: one append and one attention_flexible_paged(kernel="auto") per DISTINCT count.  Both
in this process on the same box, with HIP events.

    python tools/kv_paged_ragged_bench.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/kv_paged_ragged.json]

Shapes (fp16, Llama-7B's heads 32 / 32, d = 128, causal; the lengths are those BEFORE the step, every sequence then takes its count):
    15 decoders at 4101 keys plus one chunk of 512 rows on 1029 keys;
    63 decoders at 1029 keys plus two chunks of 256 rows on 16 and on 2053 keys.
The method is tools/kv_paged_bench.py's: the legs alternate over several rounds and every round is reported; `timed` and the buffer
rotation are tools/attn_bench.py's (distinct pools beyond the Infinity Cache); what is timed is a CALL as a user makes it, Python,
metadata copies and launches included.  The timed step is repeated at one length: the host lengths are set back before it.  A
repeated append does the same work on the same pages, but a chunk that leaves an open block behind has overwritten the staging rows
its repeat reads, so from the second time on the chunk's first block of K holds other values: the comparison of the two legs' outputs
is therefore made once, on two pools built alike, one per leg, before anything is repeated.
Per shape: microseconds per leg (median of the rounds) and every round, the baseline's spread, the ratio, whether both legs give the
same bits, and the launches of each leg.  No ratio is a pass condition: the numbers are recorded; the tool exits non-zero only when
the outputs differ.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
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
from lqer_amd import PagedKVCache, attention_flexible_paged, attention_flexible_paged_ragged  # noqa: E402

H, HK, D = 32, 32, 128
# name, [(sequences, keys before the step, count)]: the groups in the order the step names them
SHAPES = [("dec15_t4101_chunk512_t1029", [(15, 4101, 1), (1, 1029, 512)]),
          ("dec63_t1029_chunks256_t16_t2053", [(63, 1029, 1), (1, 16, 256), (1, 2053, 256)])]
LEGS = ("per_count", "ragged")


def one_shape(name, groups, cfg, a):
    dt = torch.float16
    have = [t for n, t, _ in groups for _ in range(n)]
    counts = [c for n, _, c in groups for _ in range(n)]
    lens = [t + c for t, c in zip(have, counts)]
    b, total = len(have), sum(counts)
    pages = sum((n + 15) // 16 for n in lens)
    stride = (max(lens) + 15) // 16
    pool_bytes = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride).nbytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // pool_bytes)))  # the rotation spans three times the Infinity Cache
    by_count = {}  # count -> the step's sequences that take it (the baseline's calls)
    for i, c in enumerate(counts):
        by_count.setdefault(c, []).append(i)
    at = [sum(counts[:i]) for i in range(b)]
    g = torch.Generator(device="cuda")

    def make(seed):
        g.manual_seed(seed)
        paged = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)
        seqs = [paged.alloc() for _ in have]
        for sq, n in zip(seqs, have):
            k, v = (torch.randn(1, HK, n, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
            paged.append([sq], k, v)
            del k, v
        q, kn, vn = (torch.randn(total, heads, D, generator=g, device="cuda", dtype=dt) for heads in (H, HK, HK))
        # the baseline's tensors, [sequences, heads, count, d] per distinct count: the same values
        split = {c: tuple(torch.stack([x[at[i]:at[i] + c].transpose(0, 1) for i in idx]).contiguous() for x in (q, kn, vn)) for c, idx in by_count.items()}
        past = {paged.pt.slot(s): n for s, n in zip(seqs, have)}  # the host lengths the timed step starts from
        return paged, seqs, q, kn, vn, split, past

    bufs = [make(len(name) + i) for i in range(nbuf)]
    scaling = D ** -0.5

    def rewind(paged, past):
        for slot, n in past.items():
            paged.pt.lengths[slot] = n

    def per_count(paged, seqs, q, kn, vn, split, past):  # one append and one attention per distinct count
        rewind(paged, past)
        for c, idx in by_count.items():
            paged.append([seqs[i] for i in idx], split[c][1], split[c][2])
        return [attention_flexible_paged(split[c][0], paged, [seqs[i] for i in idx], scaling, causal=True, out_layout="bshd", kernel="auto")
                for c, idx in by_count.items()]

    def ragged(paged, seqs, q, kn, vn, split, past):
        rewind(paged, past)
        paged.append_ragged(seqs, kn, vn, counts)
        return attention_flexible_paged_ragged(q, paged, seqs, counts, scaling, causal=True)

    fns = {"per_count": per_count, "ragged": ragged}
    # the same step on two pools made alike, one per leg (a chunk's append is not repeatable on ONE pool: see the docstring)
    want, got = per_count(*make(7)), ragged(*make(7))
    same = all(bool(torch.equal(w[j], got[at[i]:at[i] + c])) for w, (c, idx) in zip(want, by_count.items()) for j, i in enumerate(idx))
    del want, got
    torch.cuda.empty_cache()
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    small = sorted(c for c in by_count if c <= 8)
    big = [c for c in by_count if c > 8]
    out = {"shape": name, "sequences": b, "groups": [{"sequences": n, "keys_before": t, "count": c} for n, t, c in groups], "rows": total,
           "heads_kvheads_d": [H, HK, D], "dtype": "float16", "mask": "causal", "buffers": nbuf, "pool_bytes": pool_bytes, "same_bits": same,
           # library launches: an append is 1; an attention call is 3 (the decode kernels, or K image + V image + k_attn_q)
           "per_count_launches": {"append": len(by_count), "attention": 3 * len(by_count)},
           # (all sequences of up to 8 rows are one call, the chunks another; the groups' rows are ranges of q here: nothing is gathered,
           # and both calls write their rows of out in place)
           "ragged_launches": {"append": 1, "attention": (3 if small else 0) + (3 if big else 0), "torch_copies_into_out": 0}}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    out["per_count_rounds_spread_frac"] = round((max(rounds["per_count"]) - min(rounds["per_count"])) / med["per_count"], 4)
    out["ragged_over_per_count"] = round(med["ragged"] / med["per_count"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_ragged.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_ragged_bench.py needs a GPU (no fall-back)")
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
    ok = all(x["same_bits"] for x in shapes)
    out = {"tool": "tools/kv_paged_ragged_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call (Python, metadata copies, launches) included; a step = "
           "append of every sequence's count of keys + causal attention of as many query rows",
           "criterion": "none on the times - both legs are recorded; every sequence's output the same bits on both legs", "same_bits": ok,
           "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("an output of the ragged leg differs from the per-count leg's")


if __name__ == "__main__":
    main()

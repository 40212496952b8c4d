"""Time the rotary position embedding of one layer's q and k plus the append of k and v to the paged KV pool, done in ONE launch
(PagedKVCache.append_ragged_rope: lqer_kv_pool_append_rope, csrc/kv_rope.hip) against the way a serving loop did it before, on the same
commit: positions from the host books, cos / sin gathered, HF's apply_rotary_pos_emb on q and k in torch, then append_ragged.  Both in
this process on the same box, with HIP events.

    python tools/kv_rope_bench.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/kv_rope.json]

Shapes (fp16, d = 128, heads 32 / 32 and 32 / 8; the lengths are those BEFORE the step): decode steps of 8 and of 64 sequences at 1029
and at 4101 keys, and a mixed step - 63 decoders at 1029 keys plus one chunk of 512 rows on 1029 keys.
The method is tools/kv_paged_ragged_bench.py's: the legs alternate over several rounds and every round is reported; `timed` and the
buffer rotation are tools/attn_bench.py's (distinct pools and operands beyond the Infinity Cache); what is timed is a CALL as a user
makes it, Python, metadata copies and launches included; the host lengths are set back before every timed step.  The torch leg is the
reference: the fused leg's rotated queries and the keys it left in the pool must be the same bits, checked once on two pools built
alike.  Per shape and leg: milliseconds (median of the rounds) and every round, the device launches and copies a call makes (by
construction), the bytes its kernels read and write (from the shapes), the reference's spread and the ratio.  No ratio is a pass
condition and nothing routes on one: the tool exits non-zero only when the bits differ.  Not part of bench.py.  Needs a GPU: there is
no fall-back."""
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
from lqer_amd import PagedKVCache, rope_tables  # noqa: E402

D, ROWS = 128, 8192
# name, heads, kv heads, [(sequences, keys before the step, count)]
SHAPES = [(f"dec{b}_t{t}_h{h}_{hk}", h, hk, [(b, t, 1)]) for b in (8, 64) for t in (1029, 4101) for h, hk in ((32, 32), (32, 8))]
SHAPES.append(("dec63_t1029_chunk512_t1029_h32_8", 32, 8, [(63, 1029, 1), (1, 1029, 512)]))
LEGS = ("torch", "fused")


def leg_bytes(total, h, hk, seqs_blocks, counts):
    """Bytes the kernels of each leg read and write, from the shapes (fp16; metadata aside)."""
    nq, nk, c = total * h * D * 2, total * hk * D * 2, total * D * 2  # q, k (= v), one gathered [total, D] table
    # the append: v read; per (sequence, kv head) the touched blocks' K codes and exponents written, the new V rows' codes and exponents,
    # the staging rows of the open block read and those of the new keys written (at most 16 rows each)
    pool = sum(hk * (blocks * (16 * D + D) + n * (D + D // 16) + (16 + min(n, 16)) * D * 2) for blocks, n in zip(seqs_blocks, counts))
    # HF per tensor of N bytes: neg (N/2 + N/2), cat (N + N), two multiplies (N + table + N each), add (2 N + N); two gathers of a table
    torch_rope = 10 * (nq + nk) + 4 * c + 4 * c
    return {"torch": torch_rope + nk + nk + pool, "fused": 2 * nq + nk + c + nk + pool}


def one_shape(name, h, hk, groups, cfg, rot, a):
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb

    dt = torch.float16
    have = [t for n, t, _ in groups for _ in range(n)]
    counts = [c for n, _, c in groups for _ in range(n)]
    lens = [t + c for t, c in zip(have, counts)]
    b, total = len(have), sum(counts)
    pages, stride = sum((n + 15) // 16 for n in lens), (max(lens) + 15) // 16
    pool_bytes = PagedKVCache(pages, b, hk, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride).nbytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // pool_bytes)))  # the rotation spans three times the Infinity Cache
    rope = rope_tables(rot, ROWS, dt, "cuda")
    cos_full, sin_full = (x[0] for x in rot(torch.empty(0, dtype=dt, device="cuda"), torch.arange(ROWS, device="cuda")[None]))  # HF's [rows, D]
    g = torch.Generator(device="cuda")

    def make(seed):
        g.manual_seed(seed)
        paged = PagedKVCache(pages, b, hk, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)
        seqs = [paged.alloc() for _ in have]
        for sq, n in zip(seqs, have):
            k, v = (torch.randn(1, hk, n, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
            paged.append([sq], k, v)
            del k, v
        q, kn, vn = (torch.randn(total, heads, D, generator=g, device="cuda", dtype=dt) for heads in (h, hk, hk))
        past = {paged.pt.slot(s): n for s, n in zip(seqs, have)}  # the host lengths the timed step starts from
        return paged, seqs, q, kn, vn, past

    def rewind(paged, past):
        for slot, n in past.items():
            paged.pt.lengths[slot] = n

    def leg_torch(paged, seqs, q, kn, vn, past):
        rewind(paged, past)
        pos = torch.tensor([paged.length(s) + j for s, c in zip(seqs, counts) for j in range(c)], device="cuda")  # positions from the host books
        q_rot, k_rot = apply_rotary_pos_emb(q, kn, cos_full[pos], sin_full[pos], unsqueeze_dim=1)
        paged.append_ragged(seqs, k_rot, vn, counts)
        return q_rot

    def leg_fused(paged, seqs, q, kn, vn, past):
        rewind(paged, past)
        return paged.append_ragged_rope(seqs, q, kn, vn, counts, rope)

    fns = {"torch": leg_torch, "fused": leg_fused}
    # the same step on two pools made alike, one per leg (a chunk's append is not repeatable on ONE pool: kv_paged_ragged_bench.py)
    ref, got = make(7), make(7)
    same = bool(torch.equal(leg_torch(*ref), leg_fused(*got)))
    for s in (ref[1][0], ref[1][-1]):
        same = same and all(bool(torch.equal(x, y)) for x, y in zip(ref[0].dequantized(s), got[0].dequantized(s)))
    del ref, got
    torch.cuda.empty_cache()
    bufs = [make(len(name) + i) for i in range(nbuf)]
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup) / 1e3)  # ms
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    nbytes = leg_bytes(total, h, hk, [(t + c - 1) // 16 - t // 16 + 1 for t, c in zip(have, counts)], counts)
    out = {"shape": name, "sequences": b, "groups": [{"sequences": n, "keys_before": t, "count": c} for n, t, c in groups], "rows": total,
           "heads_kvheads_d": [h, hk, D], "dtype": "float16", "buffers": nbuf, "pool_bytes": pool_bytes, "same_bits": same,
           # device work of one call: host-to-device copies (positions; slots, lengths and starts of the append), torch kernels (two gathers;
           # per tensor neg, cat, two multiplies, an add) and library launches
           "torch_launches": {"h2d_copies": 1 + 3, "torch_kernels": 2 + 2 * 5, "library": 1},
           "fused_launches": {"h2d_copies": 3, "torch_kernels": 0, "library": 1}}
    for leg in LEGS:
        out[f"ms_{leg}"] = round(med[leg], 4)
        out[f"ms_{leg}_rounds"] = [round(x, 4) for x in rounds[leg]]
        out[f"bytes_{leg}"] = nbytes[leg]
    out["torch_rounds_spread_frac"] = round((max(rounds["torch"]) - min(rounds["torch"])) / med["torch"], 4)
    out["fused_rounds_spread_frac"] = round((max(rounds["fused"]) - min(rounds["fused"])) / med["fused"], 4)
    out["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_rope.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_rope_bench.py needs a GPU (no fall-back)")
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    rot = LlamaRotaryEmbedding(LlamaConfig(hidden_size=32 * D, num_attention_heads=32, max_position_embeddings=ROWS))
    shapes = []
    with torch.no_grad():
        for sh in SHAPES:
            shapes.append(one_shape(*sh, cfg, rot, a))
            torch.cuda.empty_cache()
    ok = all(x["same_bits"] for x in shapes)
    out = {"tool": "tools/kv_rope_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call (Python, metadata copies, launches) included; a step = "
           "rotary embedding of q and k at every new token's position + append of every sequence's count of keys",
           "criterion": "none on the times - both legs are recorded, the torch leg is the reference; rotated queries and pooled keys the same "
           "bits on both legs", "same_bits": ok, "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the fused leg's bits differ from the torch leg's")


if __name__ == "__main__":
    main()

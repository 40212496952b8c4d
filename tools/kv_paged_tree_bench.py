"""Time the attention of one TREE-VERIFY step of speculative decoding over the paged KV pool - every sequence holds its committed
context plus the nodes of a draft tree as its last keys, and every node attends to the context, itself and its ancestors - done in
one attention_flexible_paged_tree call (lqer_attention_q_decode_paged_tree for trees of up to 8 nodes, lqer_attention_q_paged_tree
beyond), against the only exact route there was before the pool took a tree: per sequence, PagedKVCache.to_dense() - a gather of the
whole sequence into a dense cache - plus attention_flexible_cached(attention_mask=M) on it with the tree as a mask tensor.  Both in
this process on the same box, with HIP events.

    python tools/kv_paged_tree_bench.py [--steps 5] [--warmup 2] [--rounds 3] [--out profiles/kv_paged_tree.json]

Shapes (fp16, Llama-7B's heads 32 / 32, d = 128; the lengths include the draft nodes):
    16 and 64 sequences, of 1029 and of 4101 keys each (all four pairs), each with
      a binary tree of 8 nodes (the decode route), a tree of 26 nodes - two roots, fan-out 3, three levels - and one of 60 nodes - the
      same rule, a fourth level begun - (the prefill route).
The append of the draft keys (append_ragged) is the same launch on both legs and is not timed; the mask tensors of the per-sequence
leg are built once, outside the timing.  The timing is tools/kv_paged_spec_bench.py's: the legs alternate over several rounds and
every round is reported; `timed` and the buffer rotation are tools/attn_bench.py's (distinct pools beyond the Infinity Cache); what
is timed is a CALL as a user makes it, Python, metadata copies and launches included.  The two legs' outputs are compared once.
Per shape: microseconds per leg (median of the rounds) and every round, the ratio, whether both legs give the same bits, and the
library launches and the bytes copied of each leg - those two by construction, from the calls each leg makes and the size of a dense
cache, not from counters.  No ratio is a pass condition: the numbers are recorded; the tool exits non-zero
only when the outputs differ.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
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
from lqer_amd import PagedKVCache, attention_flexible_cached, attention_flexible_paged_tree, tree_masks  # noqa: E402

H, HK, D = 32, 32, 128
LEGS = ("dense_per_sequence", "one_call")
fan3 = lambda n: [-1 if i < 2 else (i - 2) // 3 for i in range(n)]  # two roots, every node three children, in breadth-first order
TREES = {"binary8": [(i - 1) // 2 for i in range(8)], "fan3_26": fan3(26), "fan3_60": fan3(60)}
# name, sequences, keys (the draft nodes included)
SIZES = [(f"b{b}_t{t}", b, t) for b in (16, 64) for t in (1029, 4101)]


def mask_tensor(t, parents, dt):
    """[1, 1, n, t]: 0 where node i sees key j, the most negative finite value elsewhere."""
    n = len(parents)
    m = torch.full((n, t), torch.finfo(dt).min, dtype=dt)
    m[:, :t - n] = 0
    for i, w in enumerate(tree_masks(parents)):
        for j in range(i + 1):
            if w >> j & 1:
                m[i, t - n + j] = 0
    return m.view(1, 1, n, t).cuda()


def one_size(name, b, t, cfg, a):
    dt = torch.float16
    pages, stride = b * ((t + 15) // 16), (t + 15) // 16
    pool_bytes = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride).nbytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // pool_bytes)))  # the rotation spans three times the Infinity Cache
    g = torch.Generator(device="cuda")
    n_max = max(map(len, TREES.values()))

    def make(seed):
        g.manual_seed(seed)
        paged = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)
        seqs = [paged.alloc() for _ in range(b)]
        for sq in seqs:
            k, v = (torch.randn(1, HK, t, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
            paged.append([sq], k, v)
            del k, v
        return paged, seqs, torch.randn(b * n_max, H, D, generator=g, device="cuda", dtype=dt)

    bufs = [make(len(name) + i) for i in range(nbuf)]
    scaling = D ** -0.5
    out = []
    for tree, parents in TREES.items():
        n = len(parents)
        mask = mask_tensor(t, parents, dt)
        kernel = "decode" if n <= 8 else "prefill"

        def dense_per_sequence(paged, seqs, q):
            """The exact route without a tree entry: every sequence gathered into a dense cache, one masked call each."""
            res = torch.empty(b * n, H, D, dtype=dt, device=q.device)
            for i, sq in enumerate(seqs):
                res[i * n:(i + 1) * n] = attention_flexible_cached(q[i * n:(i + 1) * n].transpose(0, 1)[None], paged.to_dense(sq), scaling, attention_mask=mask,
                                                                   out_layout="bshd", kernel=kernel)[0]
            return res

        def one_call(paged, seqs, q):
            return attention_flexible_paged_tree(q[:b * n], paged, seqs, [parents] * b, scaling)

        fns = {"dense_per_sequence": dense_per_sequence, "one_call": one_call}
        want, got = dense_per_sequence(*bufs[0]), one_call(*bufs[0])
        same = bool(torch.equal(want, got))
        del want, got
        rounds = {leg: [] for leg in LEGS}
        for _ in range(a.rounds):
            for leg in LEGS:
                rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
        med = {leg: statistics.median(v) for leg, v in rounds.items()}
        plan = attention_flexible_paged_tree.plan(bufs[0][0], bufs[0][1], [parents] * b)
        dense_bytes = bufs[0][0].to_dense(bufs[0][1][0]).nbytes
        res = {"shape": f"{name}_{tree}", "sequences": b, "keys": t, "tree": tree, "nodes": n, "parents": parents, "rows": b * n,
               "heads_kvheads_d": [H, HK, D], "dtype": "float16", "route": kernel, "buffers": nbuf, "pool_bytes": pool_bytes, "same_bits": same,
               # BY CONSTRUCTION, not observed - library launches: to_dense is 1 gather; an attention call is 3 (decode: scores, PV, sum;
               # prefill: two images, the kernel)
               "launches_and_bytes": "by construction: counted from the calls each leg makes and the size of a dense cache, not measured",
               "dense_per_sequence_launches": {"gather": b, "attention_calls": b, "attention": 3 * b},
               "one_call_launches": {"gather": 0, "attention_calls": len(plan), "attention": 3 * len(plan)},
               "one_call_plan": plan,
               # device-to-device copies of keys and values; the one call sends the rows' 8-byte masks from the host instead
               "dense_per_sequence_bytes_copied": b * dense_bytes, "one_call_bytes_copied": 0, "one_call_mask_bytes_from_host": 8 * b * n}
        for leg in LEGS:
            res[f"us_{leg}"] = round(med[leg], 1)
            res[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
        res["one_call_over_dense_per_sequence"] = round(med["one_call"] / med["dense_per_sequence"], 4)
        out.append(res)
        print(f"{res['shape']}: dense_per_sequence {res['us_dense_per_sequence']} us, one_call {res['us_one_call']} us, same bits {same}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_tree.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_tree_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    shapes = []
    with torch.no_grad():
        for sz in SIZES:
            shapes += one_size(*sz, cfg, a)
            torch.cuda.empty_cache()
    ok = all(x["same_bits"] for x in shapes)
    out = {"tool": "tools/kv_paged_tree_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call (Python, metadata copies, launches) included; what is "
           "timed is the attention of a verify step - the append of the draft keys is common to both legs and left out",
           "criterion": "none on the times - both legs are recorded; every sequence's output the same bits on both legs", "same_bits": ok,
           "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("an output of the one-call leg differs from the per-sequence leg's")


if __name__ == "__main__":
    main()

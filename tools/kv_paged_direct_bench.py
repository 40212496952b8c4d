"""Time the prefill kernel that reads the paged pool's codes in its key loop (kernel="direct": lqer_attention_q_paged_direct, ONE launch,
no workspace) against the image route (kernel="prefill": k_kv_kimage + k_kv_vimage + k_attn_q, a workspace that follows the longest
addressed length) on the same pool and the same queries, in this process, with HIP events.

    python tools/kv_paged_direct_bench.py [--steps 10] [--warmup 3] [--rounds 5] [--only tree,ragged,window] [--out profiles/kv_paged_direct.json]

Shapes (fp16, Llama-7B's heads 32 / 32, d = 128), taken from the tools that timed the image route:
    tree    tools/kv_paged_tree_bench.py's verify step: 16 and 64 sequences of 1029 and 4101 keys, trees of 26 and 60 nodes;
    ragged  tools/kv_paged_ragged_bench.py's mixed steps (15 decoders at 4101 keys + a 512-row chunk at 1029; 63 decoders at 1029 + two
            256-row chunks at 16 and 2053), every sequence - the decoders' single rows too - through the ONE call of either kernel;
    window  tools/kv_paged_window_prefill_bench.py's 512-row chunk, batch 8, under W = 1024 at 4101 and 16389 keys (old pages released).
Timing is tools/attn_bench.py's `timed` and buffer rotation (distinct pools spanning three times the Infinity Cache, warm-up calls on
every shape first); the two legs alternate over several rounds, every round is reported and the median is the figure.  What is timed is
a CALL as a user makes it: Python, metadata copies and launches included.  Per shape and leg: ms, library launches, workspace bytes (the
library's own size functions) and the bytes moved - the last BY CONSTRUCTION from the shapes (codes 1 B / element with an exponent
byte per 16; images 2 B / element written once and read twice for K, once for V, per query tile and head), not from counters.  The two
legs' outputs are compared once: the tool exits non-zero only when they differ.  No ratio is a pass condition.  Not part of bench.py.
Needs a GPU: there is no fall-back."""
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
from lqer_amd import PagedKVCache, _lib, attention_flexible_paged_ragged, attention_flexible_paged_tree  # noqa: E402

H, HK, D = 32, 32, 128
LEGS = ("prefill", "direct")
fan3 = lambda n: [-1 if i < 2 else (i - 2) // 3 for i in range(n)]
TREES = {"fan3_26": fan3(26), "fan3_60": fan3(60)}
RAGGED = [("dec15_t4101_chunk512_t1029", [(15, 4101, 1), (1, 1029, 512)]),
          ("dec63_t1029_chunks256_t16_t2053", [(63, 1029, 1), (1, 16, 256), (1, 2053, 256)])]
WINDOW, CHUNK, WB = 1024, 512, 8


def pools(lens, cfg, window=None):
    """Enough pools alike - sequences of `lens` keys, grown in appends of up to CHUNK under a window - that a rotation spans the cache."""
    dt, stride = torch.float16, (max(lens) + 15) // 16
    kw = dict(window=window, max_query_rows=CHUNK) if window else {}
    pages = len(lens) * ((window + CHUNK + 29) // 16) if window else sum((n + 15) // 16 for n in lens)
    g = torch.Generator(device="cuda")

    def make(seed):
        g.manual_seed(seed)
        paged = PagedKVCache(pages, len(lens), HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride, **kw)
        seqs = [paged.alloc() for _ in lens]
        for sq, n in zip(seqs, lens):
            for at in range(0, n, CHUNK if window else n):
                k, v = (torch.randn(1, HK, min(CHUNK if window else n, n - at), D, generator=g, device="cuda", dtype=dt) for _ in range(2))
                paged.append([sq], k, v)
        return paged, seqs

    first = make(1)
    nbuf = max(3, min(64, -(-3 * L3_BYTES // first[0].nbytes)))
    return [first] + [make(2 + i) for i in range(nbuf - 1)]


def moved(lens, counts, window=None):
    """Bytes by construction, per leg: (codes and exponents read, image bytes written, bytes the attention kernel reads)."""
    code = lambda t: t * D * 17 // 16
    conv = sum(2 * HK * code(t) for t, c in zip(lens, counts) if c)
    seen = [min(t, window + c) if window else t for t, c in zip(lens, counts)]
    tiles = [-(-c // 128) for c in counts]
    return {"prefill": {"codes_read": conv, "image_written": sum(HK * 4 * t * D for t, c in zip(lens, counts) if c),
                        "kernel_read": sum(H * n * 6 * t * D for t, n in zip(seen, tiles))},
            "direct": {"codes_read": sum(H * n * 3 * code(t) for t, n in zip(seen, tiles)), "image_written": 0, "kernel_read": 0}}


def measure(name, bufs, q, call, lens, counts, a, window=None, extra=None):
    """Both legs of one shape: call(kernel, paged, seqs, q) is the user's call."""
    fns = {leg: (lambda paged, seqs, leg=leg: call(leg, paged, seqs, q)) for leg in LEGS}
    want, got = (fns[leg](*bufs[0]) for leg in LEGS)
    same = bool(torch.equal(want, got))
    del want, got
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    L, b = _lib.lib(), len(lens)
    max_len = min((max(lens) + 127) // 128 * 128, bufs[0][0].pt.max_len)
    ws = {"prefill": L.lqer_attention_q_paged_ragged_workspace_bytes(b, H, HK, max(counts), max_len, D),
          "direct": L.lqer_attention_q_paged_direct_workspace_bytes(b, H, HK, max(counts), max_len, D)}
    by = moved(lens, counts, window)
    res = {"shape": name, "sequences": b, "rows": sum(counts), "heads_kvheads_d": [H, HK, D], "dtype": "float16", "buffers": len(bufs), "same_bits": same,
           "bytes_moved": "by construction from the shapes, not measured", **(extra or {})}
    for leg in LEGS:
        res[leg] = {"ms": round(med[leg] / 1e3, 4), "ms_rounds": [round(x / 1e3, 4) for x in rounds[leg]], "launches": 3 if leg == "prefill" else 1,
                    "workspace_bytes": ws[leg], "bytes_moved": by[leg], "bytes_moved_total": sum(by[leg].values())}
    res["direct_over_prefill"] = round(med["direct"] / med["prefill"], 4)
    print(f"{name}: prefill {res['prefill']['ms']} ms, direct {res['direct']['ms']} ms, ratio {res['direct_over_prefill']}, same bits {same}", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="tree,ragged,window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_direct.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_direct_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    dt, scaling, shapes, only = torch.float16, D ** -0.5, [], a.only.split(",")
    g = torch.Generator(device="cuda").manual_seed(11)
    rand_q = lambda rows: torch.randn(rows, H, D, generator=g, device="cuda", dtype=dt)
    with torch.no_grad():
        for b in (16, 64) if "tree" in only else ():
            for t in (1029, 4101):
                bufs = pools([t] * b, cfg)
                for tree, parents in TREES.items():
                    call = lambda kernel, paged, seqs, q, p=parents: attention_flexible_paged_tree(q, paged, seqs, [p] * len(seqs), scaling, kernel=kernel)
                    shapes.append(measure(f"tree_b{b}_t{t}_{tree}", bufs, rand_q(b * len(parents)), call, [t] * b, [len(parents)] * b, a,
                                          extra={"family": "tree", "keys": t, "nodes": len(parents)}))
                del bufs
                torch.cuda.empty_cache()
        for name, groups in RAGGED if "ragged" in only else ():
            counts = [c for n, _, c in groups for _ in range(n)]
            lens = [t + c for n, t, c in groups for _ in range(n)]
            bufs = pools(lens, cfg)
            call = lambda kernel, paged, seqs, q, cs=counts: attention_flexible_paged_ragged(q, paged, seqs, cs, scaling, causal=True, kernel=kernel)
            shapes.append(measure(f"ragged_{name}", bufs, rand_q(sum(counts)), call, lens, counts, a,
                                  extra={"family": "ragged", "groups": [{"sequences": n, "keys_before": t, "count": c} for n, t, c in groups]}))
            del bufs
            torch.cuda.empty_cache()
        for t in (4101, 16389) if "window" in only else ():
            bufs = pools([t] * WB, cfg, window=WINDOW)
            call = lambda kernel, paged, seqs, q: attention_flexible_paged_ragged(q, paged, seqs, [CHUNK] * WB, scaling, causal=True, kernel=kernel)
            shapes.append(measure(f"window_t{t}_w{WINDOW}_chunk{CHUNK}", bufs, rand_q(WB * CHUNK), call, [t] * WB, [CHUNK] * WB, a, window=WINDOW,
                                  extra={"family": "window", "keys": t, "window": WINDOW}))
            del bufs
            torch.cuda.empty_cache()
    ok = all(x["same_bits"] for x in shapes)
    out = {"tool": "tools/kv_paged_direct_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "legs": list(LEGS), "timing": "eager calls between HIP events, the legs alternating over the rounds, the median reported: "
           "the host side of a call (Python, metadata copies, launches) is included", "criterion": "none on the times; the two legs give the same bits",
           "same_bits": ok, "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("the direct kernel's output differs from the image route's")


if __name__ == "__main__":
    main()

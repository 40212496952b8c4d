"""Time one VERIFY step of speculative decoding over the paged KV pool - every sequence appends its own number of draft tokens (1 .. 8)
and attends with as many query rows - done in one append_ragged plus one attention_flexible_paged_ragged(causal=True), which now puts
all sequences of up to 8 rows into ONE lqer_attention_q_decode_paged_ragged call, against the same step with the attention done the
way that route worked before per-sequence counts reached the decode kernels, rebuilt from calls that still exist: one
attention_flexible_paged(kernel="decode") per DISTINCT count, its rows gathered by index and its output scattered back.  Both in this
process on the same box, with HIP events.

    python tools/kv_paged_spec_bench.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/kv_paged_spec.json]

Shapes (fp16, Llama-7B's heads 32 / 32, d = 128, causal; the lengths are those BEFORE the step, every sequence then takes its count):
    16 sequences at 4101 keys and 64 sequences at 1029 keys, each with
      counts drawn once from a fixed seed in 1 .. 8 (every distinct count a call of its own on the per-count leg), and
      one token everywhere except a single sequence with 8 (continuous batching: the per-count leg's workspace follows batch x count,
      the new call's the tokens of the step).
The method is tools/kv_paged_ragged_bench.py's, and so is the timing: the legs alternate over several rounds and every round is
reported; `timed` and the buffer rotation are tools/attn_bench.py's (distinct pools beyond the Infinity Cache); what is timed is a
CALL as a user makes it, Python, metadata copies and launches included.  The timed step is repeated at one length: the host lengths
are set back before it (an append of up to 8 keys at length % 16 = 5 stays inside one open block, so the repeat does the same work on
the same bytes).  The two legs' outputs are compared once, on two pools built alike, before anything is repeated.
Per shape: microseconds per leg (median of the rounds) and every round, the baseline's spread, the ratio, whether both legs give the
same bits, and the library calls, launches and workspace bytes of each leg (attention_flexible_paged_ragged.plan for the new one).  No
ratio is a pass condition: the numbers are recorded; the tool exits non-zero only when the outputs differ.  Not part of bench.py.
Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attn_bench import L3_BYTES, timed  # noqa: E402
from lqer_amd import PagedKVCache, _lib, attention_flexible_paged, attention_flexible_paged_ragged  # noqa: E402

H, HK, D = 32, 32, 128
LEGS = ("per_count", "one_call")


def seeded_counts(b):
    rng = random.Random(1234 + b)
    return [rng.randint(1, 8) for _ in range(b)]


# name, sequences, keys before the step, counts
SHAPES = [("b16_t4101_seeded_1to8", 16, 4101, seeded_counts(16)),
          ("b16_t4101_ones_and_one_8", 16, 4101, [1] * 7 + [8] + [1] * 8),
          ("b64_t1029_seeded_1to8", 64, 1029, seeded_counts(64)),
          ("b64_t1029_ones_and_one_8", 64, 1029, [1] * 31 + [8] + [1] * 32)]


def one_shape(name, b, t, counts, cfg, a):
    dt = torch.float16
    total = sum(counts)
    lens = [t + c for c in counts]
    pages = sum((n + 15) // 16 for n in lens)
    stride = (max(lens) + 15) // 16
    pool_bytes = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride).nbytes
    nbuf = max(3, min(64, -(-3 * L3_BYTES // pool_bytes)))  # the rotation spans three times the Infinity Cache
    at = [sum(counts[:i]) for i in range(b)]
    by_count = {}  # count -> the step's sequences that take it (the per-count leg's calls)
    for i, c in enumerate(counts):
        by_count.setdefault(c, []).append(i)
    rows_of = {c: [r for i in idx for r in range(at[i], at[i] + c)] for c, idx in by_count.items()}
    g = torch.Generator(device="cuda")

    def make(seed):
        g.manual_seed(seed)
        paged = PagedKVCache(pages, b, HK, D, cfg, cfg, dt, "cuda", max_pages_per_seq=stride)
        seqs = [paged.alloc() for _ in range(b)]
        for sq in seqs:
            k, v = (torch.randn(1, HK, t, D, generator=g, device="cuda", dtype=dt) for _ in range(2))
            paged.append([sq], k, v)
            del k, v
        q, kn, vn = (torch.randn(total, heads, D, generator=g, device="cuda", dtype=dt) for heads in (H, HK, HK))
        past = {paged.pt.slot(s): t for s in seqs}  # the host lengths the timed step starts from
        return paged, seqs, q, kn, vn, past

    bufs = [make(len(name) + i) for i in range(nbuf)]
    scaling = D ** -0.5

    def rewind(paged, past):
        for slot, n in past.items():
            paged.pt.lengths[slot] = n

    def per_count(paged, seqs, q, kn, vn, past):
        """The route before this call existed: the rows of every distinct count gathered through one index tensor (copied to the device
        once), one uniform decode call per count, its output scattered back."""
        rewind(paged, past)
        paged.append_ragged(seqs, kn, vn, counts)
        out = torch.empty_like(q)
        idx = torch.tensor([r for rows in rows_of.values() for r in rows], dtype=torch.int64).to(q.device)
        lo = 0
        for c, seq_idx in by_count.items():
            ix = idx[lo:lo + len(rows_of[c])]
            lo += len(rows_of[c])
            got = attention_flexible_paged(q.index_select(0, ix).view(len(seq_idx), c, H, D).transpose(1, 2), paged, [seqs[i] for i in seq_idx], scaling,
                                           causal=True, out_layout="bshd", kernel="decode")
            out.index_copy_(0, ix, got.view(len(seq_idx) * c, H, D))
        return out

    def one_call(paged, seqs, q, kn, vn, past):
        rewind(paged, past)
        paged.append_ragged(seqs, kn, vn, counts)
        return attention_flexible_paged_ragged(q, paged, seqs, counts, scaling, causal=True)

    fns = {"per_count": per_count, "one_call": one_call}
    # the same step on two pools made alike, one per leg
    want, got = per_count(*make(7)), one_call(*make(7))
    same = bool(torch.equal(want, got))
    del want, got
    torch.cuda.empty_cache()
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(fns[leg], bufs, a.steps, a.warmup))
    med = {leg: statistics.median(v) for leg, v in rounds.items()}
    L = _lib.lib()
    plan = attention_flexible_paged_ragged.plan(bufs[0][0], bufs[0][1], counts)
    room, tight = 16 * stride, min((max(lens) + 127) // 128 * 128, 16 * stride)  # max_len of the uniform decode route / of the new call
    out = {"shape": name, "sequences": b, "keys_before": t, "counts": counts, "distinct_counts": len(by_count), "rows": total,
           "heads_kvheads_d": [H, HK, D], "dtype": "float16", "mask": "causal", "buffers": nbuf, "pool_bytes": pool_bytes, "same_bits": same,
           # library launches: an append is 1; an attention call is 3 (the decode kernels); torch: a gather and a scatter per call
           "per_count_launches": {"append": 1, "attention_calls": len(by_count), "attention": 3 * len(by_count), "torch_gather_scatter": 2 * len(by_count)},
           "one_call_launches": {"append": 1, "attention_calls": len(plan), "attention": 3 * len(plan),
                                 "torch_gather_scatter": 2 * sum(p["rows"] == "gathered" for p in plan)},
           "one_call_plan": plan,
           # (the per-count leg reuses one workspace: its largest call)
           "per_count_workspace_bytes": max(L.lqer_attention_q_decode_paged_workspace_bytes(len(idx), H, HK, c, room, D) for c, idx in by_count.items()),
           "one_call_workspace_bytes": L.lqer_attention_q_decode_paged_ragged_workspace_bytes(total, H, tight, D)}
    for leg in LEGS:
        out[f"us_{leg}"] = round(med[leg], 1)
        out[f"us_{leg}_rounds"] = [round(x, 1) for x in rounds[leg]]
    out["per_count_rounds_spread_frac"] = round((max(rounds["per_count"]) - min(rounds["per_count"])) / med["per_count"], 4)
    out["one_call_over_per_count"] = round(med["one_call"] / med["per_count"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_spec.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_spec_bench.py needs a GPU (no fall-back)")
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
    out = {"tool": "tools/kv_paged_spec_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": list(LEGS), "timing": "eager calls between HIP events: host side of a call (Python, metadata copies, launches) included; a step = "
           "append_ragged of every sequence's count of keys + causal attention of as many query rows",
           "criterion": "none on the times - both legs are recorded; every sequence's output the same bits on both legs", "same_bits": ok,
           "shapes": shapes}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not ok:
        raise SystemExit("an output of the one-call leg differs from the per-count leg's")


if __name__ == "__main__":
    main()

"""Time a decode step - the append of one key per sequence plus the causal attention of one query row per head - over a paged KV pool
that stores the codes of its 4-bit K and V formats as NIBBLES (PagedKVCache(code_bits=4): LQER_Q_MXINT_C4, two codes per byte) against
the same step over a pool of the same formats with a byte per code (code_bits=None, the pool as it was), in this process, with HIP events.

    python tools/kv_paged_nibble_bench.py [--steps 100] [--warmup 10] [--rounds 5] [--out profiles/kv_paged_nibble.json]

Llama-7B heads (32 / 32, d = 128), fp16, batch 8, histories of 4101 and 16389 keys; Q and P in the templates' 8-bit block_fp, K and V
block_fp of width 4 (8-bit exponent field, blocks of 16).  Both legs hold the same keys, quantized alike - the storage changes no
rounding, and the tool checks that the two steps give the same bits.  `kv_paged_window_bench.py`'s method: `attn_bench.py`'s `timed`,
the legs alternating over five rounds with every round reported, each leg's pools rotated over three times the Infinity Cache by the
bytes its pages hold, whole calls timed (host side included), the step repeated at one length.
Recorded next to the times, by arithmetic: both legs' pool bytes, the bytes of one page (16 keys of all kv heads, codes and exponents
of K and V), and how many pages of either kind fit a fixed budget of 16 GiB.
The claim of the nibble pool is capacity.  For time the criterion is only that the nibble leg's median is not slower than the byte
leg's by more than the byte leg's own spread - its slowest round minus its fastest; `criterion_met` records it and does not change the
exit status.  Not part of bench.py.  Needs a GPU: there is no fall-back."""
import argparse
import copy
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
from lqer_amd import PagedKVCache, attention_flexible_paged  # noqa: E402

H, HK, D, B = 32, 32, 128, 8
HISTORIES = (4101, 16389)
LEGS = {"byte": None, "nibble": 4}
BUDGET = 16 << 30


def page_bytes(bits):
    """Codes and exponents of K and V of one page - 16 keys of all kv heads: 2 x (16 D bits / 8 + D) bytes per kv head."""
    return HK * 2 * (16 * D * bits // 8 + D)


def _pool(t, bits, k, v, cfg):
    """A pool holding the first t keys of k / v [B, HK, t, D], set up so that the timed step - the append of key t - 1 - can be
    repeated: (cache, seqs, the new key's k and v, the host lengths to start from)."""
    per_seq = (t + 15) // 16
    cache = PagedKVCache(B * per_seq, B, HK, D, cfg, cfg, torch.float16, "cuda", max_pages_per_seq=per_seq, code_bits=bits)
    seqs = [cache.alloc() for _ in range(B)]
    cache.append(seqs, k, v)
    new = (k[:, :, t - 1:t].clone(), v[:, :, t - 1:t].clone())
    past = {cache.pt.slot(s): t - 1 for s in seqs}
    return cache, seqs, new, past


def one_history(t, cfg, a):
    dt, scaling = torch.float16, D ** -0.5
    g = torch.Generator(device="cuda").manual_seed(t)
    k, v = (torch.randn(B, HK, t, D, generator=g, device="cuda", dtype=dt) for _ in range(2))  # one history for every buffer
    qs = [torch.randn(B, H, 1, D, generator=g, device="cuda", dtype=dt) for _ in range(64)]
    bufs, pools = {}, {}
    for leg, bits in LEGS.items():
        first = _pool(t, bits, k, v, cfg)
        pools[leg] = first[0].nbytes
        nbuf = max(3, min(64, -(-3 * L3_BYTES // (B * ((t + 15) // 16) * page_bytes(bits or 8)))))  # three times the Infinity Cache
        bufs[leg] = [(qs[i], *p) for i, p in enumerate([first] + [_pool(t, bits, k, v, cfg) for _ in range(nbuf - 1)])]
    del k, v

    def step(q, cache, seqs, new, past):
        for slot, n in past.items():
            cache.pt.lengths[slot] = n
        cache.append(seqs, *new)
        return attention_flexible_paged(q, cache, seqs, scaling, causal=True, out_layout="bshd")

    same = bool(torch.equal(step(*bufs["byte"][0]), step(*bufs["nibble"][0])))  # (buffer 0 of both legs: the same q)
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        for leg in LEGS:
            rounds[leg].append(timed(step, bufs[leg], a.steps, a.warmup))
    med = {leg: statistics.median(x) for leg, x in rounds.items()}
    spread = max(rounds["byte"]) - min(rounds["byte"])
    return {"entry": f"t{t}", "keys": t, "batch": B, "heads_kvheads_d": [H, HK, D], "dtype": "float16", "kv_width": 4,
            "buffers_byte": len(bufs["byte"]), "buffers_nibble": len(bufs["nibble"]), "same_bits": same,
            "pool_bytes_byte": pools["byte"], "pool_bytes_nibble": pools["nibble"], "pool_bytes_ratio": round(pools["byte"] / pools["nibble"], 4),
            "us_byte": round(med["byte"], 1), "us_byte_rounds": [round(x, 1) for x in rounds["byte"]],
            "us_nibble": round(med["nibble"], 1), "us_nibble_rounds": [round(x, 1) for x in rounds["nibble"]],
            "byte_rounds_spread_us": round(spread, 1), "byte_rounds_spread_frac": round(spread / med["byte"], 4),
            "nibble_over_byte": round(med["nibble"] / med["byte"], 4), "criterion_met": bool(med["nibble"] <= med["byte"] + spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_paged_nibble.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_paged_nibble_bench.py needs a GPU (no fall-back)")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "matmul_config.json")))
    cfg["w_quantizer"] = dict(copy.deepcopy(cfg["w_quantizer"]), width=4)  # K (of Q K^T) and V (of P V): width 4; Q and P stay 8-bit
    entries = []
    with torch.no_grad():
        for t in HISTORIES:
            entries.append(one_history(t, cfg, a))
            torch.cuda.empty_cache()
    pb = {leg: page_bytes(bits or 8) for leg, bits in LEGS.items()}
    out = {"tool": "tools/kv_paged_nibble_bench.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds,
           "legs": ["byte (code_bits=None: a byte per code)", "nibble (code_bits=4: LQER_Q_MXINT_C4, two codes per byte)"],
           "timing": "eager calls between HIP events: host side of a call included; a step = append of one key per sequence + causal attention "
           "of one query row per head", "page_bytes_byte": pb["byte"], "page_bytes_nibble": pb["nibble"],
           "bytes_per_token_and_kv_head": {leg: x // (16 * HK) for leg, x in pb.items()}, "budget_bytes": BUDGET,
           "pages_in_budget_byte": BUDGET // pb["byte"], "pages_in_budget_nibble": BUDGET // pb["nibble"],
           "pages_in_budget_ratio": round(pb["byte"] / pb["nibble"], 4), "entries": entries}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    if not all(e["same_bits"] for e in entries):
        raise SystemExit("the step over the nibble pool differs from the step over the byte pool")


if __name__ == "__main__":
    main()

"""A seeded scheduler walk across every feature of the paged KV pool on the GPU, rooted in the oracle (tests/_kv_walk.py decides the
scripts on the CPU; this file only executes them on PagedKVCache).

Per form (storage and rule variant, _kv_walk.FORMS) and seed: two pools that start as 0xFF with a scrambled free stack, 70-odd ops -
alloc / free, append, append_ragged, fork, fork_many, reorder, swap_out held over some steps then swap_in (one image through
state_dict()), adopt_from the other pool and the pool itself, export + adopt, the speculation recipe, and calls that must be refused.

BEFORE EVERY STEP THAT MAY LAUNCH: check_books on the host books, and the device copy of the block table equals the host rows on every
held entry of every live slot - a broken table fails on the host and never reaches a kernel.
AFTER A REFUSED OP: it raised what the script said; the books and every byte of every pool are unchanged.
EVERY TENTH OP AND AT THE END: dequantized(seq) of every live sequence without released pages equals the oracle's block quantizer on the
model's raw K / V bit for bit (the declared |x| <= 1e-8 flush applied); one attention call per pool over its live sequences in a
shuffled order, the entry rotated by seed - attention_flexible_paged with 1 - 8 rows, kernel="prefill", shared_prefix=True,
attention_flexible_paged_decode_ragged, attention_flexible_paged_ragged (counts 0, 1 and > 8), attention_flexible_paged_tree; at the end
every entry the form allows.  out and row_stats are compared with torch.equal on the bytes against the batch-1 attention_flexible on
the model's raw tensors with the rule as a mask tensor, by the kernel the call's .plan names: the per-feature files' contract, no tolerance.
AT THE END OF FORMS X AND A: the final ragged, windowed (an explicit window of 24 keys) and tree calls against _attention.comparator on
the CPU with the same mask - O within BAR = 1e-3 relative L2 over the call's whole output; form X (integer q and K, scores exact): the
row maximum bit-equal, the row sum within 1e-6.  The comparator's own spread on those inputs is asserted <= 1e-4 in test_kv_walk_cpu.py.

A failure names form, seed, op index and op: _kv_walk.script(form, seed)[:index + 1] is the failing prefix.  The walk has exposed no
defect so far, so there is no fixed prefix case beside it."""
import time

import pytest
import torch

import _attention as A
import _formats as F
import _kv_walk as W

pytestmark = pytest.mark.gpu

DEV = A.DEV
u8 = lambda t: t.contiguous().view(torch.uint8)
to_dev = lambda t: t.to(DEV)


def _caches(form):
    from lqer_amd import PagedKVCache

    f, out = W.FORMS[form], []
    for i, kw in enumerate(W.POOLS(f)):
        cache = PagedKVCache(kw["pages"], kw["slots"], f["hk"], f["d"], f["cfg"], f["cfg"], f["dtype"], DEV, max_pages_per_seq=f["room"],
                             window=kw["window"], max_query_rows=f["rows"], code_bits=f["bits"])
        cache.buf.fill_(0xFF)
        out.append(W.scramble(form, cache, to_dev) if i < 2 else cache)
    return out


def _device_table(cache, what):
    """The device copy of the block table against the host rows, on every held entry of every live slot."""
    dev, pt = cache.table.cpu(), cache.pt
    for seq, x in pt._slot.items():
        lo, hi = pt.released[x], pt.pages_of[x]
        assert dev[x, lo:hi].tolist() == pt.table[x][lo:hi], f"{what}: the device row of sequence {seq} (slot {x}) is {dev[x, lo:hi].tolist()}, the host's {pt.table[x][lo:hi]}"


def _stored(form, caches, model, what):
    """dequantized() of every live sequence that still holds all its pages against the oracle's quantizer on the model's raw tensors."""
    f = W.FORMS[form]
    c = f["cfg"]["w_quantizer"]
    flush = lambda x: torch.where(x.abs() <= 1e-8, torch.zeros_like(x), x)
    for (p, seq), s in sorted(model.live.items()):
        if s.released or not s.keys:
            continue
        k, v = (flush(x[0].float()) for x in model.raw(p, seq))  # [hk, T, d]
        hk, t, d = k.shape
        want_k = F.oracle_q(k.transpose(1, 2).reshape(hk * d, t).contiguous(), c).reshape(hk, d, t).transpose(1, 2)  # blocks of 16 along the keys
        want_v = F.oracle_q(v.reshape(hk * t, d), c).reshape(hk, t, d)
        got_k, got_v = (x[0].cpu() for x in caches[p].dequantized(seq))
        for name, got, want in (("K", got_k, want_k), ("V", got_v, want_v)):
            assert got.shape == want.shape and torch.equal(got, want), \
                f"{what}: pool {p} sequence {seq} of {t} keys: {(got != want).sum().item()} of {want.numel()} stored {name} values differ from the oracle's"


def _kernels(cache, call, counts):
    """The comparator's kernel per sequence of a call: what the call's .plan names."""
    from lqer_amd import attention_flexible_paged_ragged, attention_flexible_paged_tree

    entry = call["entry"]
    if entry == "prefill":
        return ["prefill"] * len(counts)
    if entry in ("paged", "shared", "windowed", "decode_ragged"):
        return ["decode"] * len(counts)
    plan = (attention_flexible_paged_tree.plan(cache, call["seqs"], call["parents"]) if entry == "tree" else
            attention_flexible_paged_ragged.plan(cache, call["seqs"], counts))
    out = [None] * len(counts)
    for part in plan:
        for b in part["seqs"]:
            out[b] = "decode" if "decode" in part["call"] else "prefill"
    return out


def _attend(form, caches, model, p, call, oracle, what):
    """One attention call of a script: the bytes of out and row_stats per sequence against the comparator kernel on the model's raw
    tensors under the rule's mask tensor; `oracle`: also against the CPU comparator."""
    from lqer_amd import (attention_flexible, attention_flexible_paged, attention_flexible_paged_decode_ragged, attention_flexible_paged_ragged,
                          attention_flexible_paged_tree)

    f, cache, entry, seqs, scale = W.FORMS[form], caches[p], call["entry"], call["seqs"], W.scale_of(form)
    operands = W.call_operands(model, call)
    if entry in ("paged", "shared", "windowed", "prefill"):
        counts = [call["rows"]] * len(seqs)
        q = torch.cat([x[0] for x in operands]).to(DEV)
        out, st = attention_flexible_paged(q, cache, seqs, scale, causal=True, return_stats=True, kernel="prefill" if entry == "prefill" else "decode",
                                           shared_prefix=entry == "shared", **({"window": call["window"]} if "window" in call else {}))
        out, st = out.transpose(1, 2).reshape(-1, f["h"], f["d"]), st.transpose(1, 2).reshape(-1, f["h"], 2)  # rows [sum c, h, .]
    else:
        counts = [len(x) for x in call["parents"]] if entry == "tree" else call["counts"]
        q = torch.cat([x[0][0].transpose(0, 1) for x in operands]).contiguous().to(DEV)
        if entry == "tree":
            out, st = attention_flexible_paged_tree(q, cache, seqs, call["parents"], scale, return_stats=True)
        elif entry == "decode_ragged":
            out, st = attention_flexible_paged_decode_ragged(q, cache, seqs, counts, scale, causal=True, return_stats=True)
        else:
            out, st = attention_flexible_paged_ragged(q, cache, seqs, counts, scale, causal=True, return_stats=True)
    assert out.shape == (sum(counts), f["h"], f["d"]) and st.shape == (sum(counts), f["h"], 2)
    kernels = [k for k, c in zip(_kernels(cache, call, counts), counts) if c]
    at = 0
    for (q1, k, v, mask), kernel, (seq, c) in zip(operands, kernels, ((s, c) for s, c in zip(seqs, counts) if c)):
        want, want_st = attention_flexible(q1.to(DEV), k.to(DEV), v.to(DEV), f["cfg"], f["cfg"], scale, attention_mask=mask.to(DEV), kernel=kernel,
                                           return_stats=True)
        want, want_st = want[0].transpose(0, 1), want_st[0].transpose(0, 1)
        got, got_st = out[at:at + c], st[at:at + c]
        where = f"{what}: {call}: sequence {seq} ({k.shape[2]} keys, {c} rows, comparator kernel {kernel})"
        assert torch.equal(u8(got), u8(want)), f"{where}: {(got != want).sum().item()} of {want.numel()} outputs differ"
        assert torch.equal(u8(got_st), u8(want_st)), f"{where}: row_stats differ"
        at += c
    assert torch.isfinite(out).all(), what
    if oracle:
        ref, ref_max, ref_sum = W.oracle_reference(model, call)
        err = A._rel(out.cpu(), ref)
        line = f"{what}: {entry} on pool {p} against the CPU comparator: O rel-L2 {err:.3e}"
        stc = st.cpu()
        if f["exact"]:
            rel = float(((stc[..., 1].double() - ref_sum).abs() / ref_sum).max())
            print(f"{line}, row-sum rel {rel:.2e}, row maxima differing {(stc[..., 0] != ref_max).sum().item()}")
            assert torch.equal(stc[..., 0], ref_max), f"{line}: {(stc[..., 0] != ref_max).sum().item()} of {ref_max.numel()} row maxima differ"
            assert rel <= 1e-6, line
        else:
            print(line)
        assert err <= A.BAR, line


CASES = [(form, seed) for form in W.FORMS for seed in W.SEEDS[form]]


@pytest.mark.parametrize("form, seed", CASES, ids=[f"{f}-{s}" for f, s in CASES])
def test_walk(form, seed):
    t0 = time.time()
    ops = W.script(form, seed)
    caches, model = _caches(form), W.Model(form)
    for i, op in enumerate(ops):
        what = f"form {form} seed {seed} op {i} {op if op['op'] != 'check' else 'check'}"  # (a check's calls are named one by one)

        def before():
            for j, cache in enumerate(caches):
                W.check_books(cache.pt, model, j, what)
                _device_table(cache, what)

        final = op["op"] == "check" and op["final"]
        attend = lambda p, call: _attend(form, caches, model, p, call, final and form in W.ORACLE_FORMS and call in W.oracle_calls(ops), what)
        refused = bool(op.get("raises"))
        if refused:
            torch.cuda.synchronize()
            books, bufs = [W.books_of(c.pt) for c in caches], [c.buf.clone() for c in caches]
        try:
            W.run(dict(op), caches, model, to_dev, attend, before)
            if refused:
                torch.cuda.synchronize()
                assert [W.books_of(c.pt) for c in caches] == books, "a refused op changed the books"
                for j, (c, buf) in enumerate(zip(caches, bufs)):
                    assert torch.equal(c.buf, buf), f"a refused op changed {(c.buf != buf).sum().item()} bytes of pool {j}"
            before()
            if op["op"] == "check":
                _stored(form, caches, model, what)
        except AssertionError as e:
            raise AssertionError(str(e) if str(e).startswith(what[:what.index(" op ")]) else f"{what}: {e}") from e
        except Exception as e:
            raise AssertionError(f"{what}: {type(e).__name__}: {e}") from e
    torch.cuda.synchronize()
    print(f"walk {form}/{seed}: {len(ops)} ops in {time.time() - t0:.1f} s")

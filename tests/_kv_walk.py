"""A seeded scheduler walk over the paged KV pool, decided on the CPU: the model, the script generator, the executor and the books'
invariants that tests/test_kv_walk_cpu.py (PageTable alone) and tests/test_gpu_kv_walk.py (PagedKVCache on the GPU) share.  No GPU here.

MODEL.  For every live sequence the raw K and V it was ever given - as a list of (tensor seed, draw size, row): draw() makes the tensors,
in the pool's dtype - and its released count as PagedKVCache's docstring gives the window rule: an append of c > 0 keys to a sequence of
T keys releases the pages wholly below min(T + c - W - (R - 1), 16 (T // 16)), R = max_query_rows or 8.  Per page of every pool, WHAT the
page holds: the identities of the keys of the block that was written there.  A K quantizer block is the 16 keys of one page, so a page's
content is the tuple of its keys' identities; an append rewrites the block at T // 16 and those after it, a fork writes the child's open
block, a copy carries the content over.  check_books() then asks of the host books: lengths, pages_of = ceil(len / 16), released as the
model has it and <= len // 16, a page's owner count = the live rows that hold it, the free stack = the pages nobody holds (each once),
slots partition into free and live, every held entry of every live row names a page whose content is that block of that sequence - a
page reused while someone still reads it fails there - and no write lands on a page with a second owner.

SCRIPT.  script(form, seed) drives two HostPools (PagedKVCache's host side on a PageTable alone, written from the docstrings) plus the
model with random.Random and returns the list of ops it performed: every op names its pool, its sequences (ids are handed out in order,
so they are the same in every replay), counts, tensor seeds, the ids it creates and - `raises` - the exception a refused op must
raise.  Every tenth op and the last are `check` ops: the attention calls to make there, entries rotated by seed.  run() executes one op
on any pair of pools with PagedKVCache's methods - the HostPools here, the real caches in the GPU file - and keeps the model in step."""
from __future__ import annotations

import functools
import random

import torch

import _attention as A
import _formats as F
from lqer_amd.kvcache import PageTable

PAGE = 16
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
_X8, _W4 = F.cfg("e8", 8, [1, 16], True), F.cfg("e8", 4, [1, 16], True)
CFG8 = A.CFG                                                                # the golden config: K and V of width 8
CFG4 = dict(name="flexible", default=_X8, x_quantizer=_X8, w_quantizer=_W4)  # test_gpu_kv_swap's: K and V of width 4
# form -> the storage and rule variant.  pages: of the two pools; room: max_pages_per_seq; rows: max_query_rows
FORMS = {
    "A": dict(dtype=F16, d=48, h=4, hk=2, bits=None, window=None, rows=None, cfg=CFG8, pages=(40, 24), room=20, exact=False),
    "B": dict(dtype=BF16, d=64, h=8, hk=2, bits=None, window=20, rows=None, cfg=CFG8, pages=(24, 24), room=8, exact=False),
    "C": dict(dtype=F32, d=16, h=2, hk=1, bits=None, window=24, rows=16, cfg=CFG8, pages=(24, 24), room=8, exact=False),
    "D": dict(dtype=BF16, d=128, h=4, hk=2, bits=(4, 4), window=None, rows=None, cfg=CFG4, pages=(24, 24), room=8, exact=False),
    "E": dict(dtype=BF16, d=128, h=4, hk=2, bits=(8, 4), window=20, rows=None, cfg=CFG4, pages=(24, 24), room=8, exact=False),
    "X": dict(dtype=F16, d=64, h=4, hk=2, bits=None, window=None, rows=None, cfg=CFG8, pages=(24, 24), room=8, exact=True),
}
# (form A's first pool has 40 pages: the sequence that crosses 256 keys takes 17 of them, its fork more, and the walk needs the rest)
SLOTS = 6
# the seeds the GPU file runs, chosen on the CPU alone: the first three per form whose scripts meet unmet()'s conditions (and, for the
# forms compared with the reference, whose comparator spread is at most 1e-4) - tests/test_kv_walk_cpu.py asserts both for these very seeds
SEEDS = {"A": (1, 2, 3), "B": (0, 2, 19), "C": (1, 3, 6), "D": (2, 3, 4), "E": (3, 4, 13), "X": (0, 2, 3)}
ORACLE_FORMS = ("X", "A")  # whose final ragged, windowed and tree calls are compared with the CPU comparator
ORACLE_WINDOW = 24         # the explicit window of the final windowed call of those (their caches have none)
STEPS = 72
EXC = {"RuntimeError": RuntimeError, "KeyError": KeyError, "ValueError": ValueError}
KINDS = ("alloc", "free", "append", "append_ragged", "fork", "fork_many", "reorder", "swap_out", "swap_in", "adopt_from", "export_adopt", "spec")
REFUSALS = ("pages", "room", "freed", "window", "rows")  # out of pages; beyond max_pages_per_seq; a freed id; another window; too many rows
chunk_of = lambda t: 16 * min(max((t + 255) // 256, 1), 8)  # the decode kernels' chunk of keys for a sequence of t keys
ceil16 = lambda n: (n + PAGE - 1) // PAGE


def scale_of(form) -> float:
    """The softmax scaling of a form's calls: d^-1/2; the exact form a power of two below it, so that integer scores stay exact."""
    f = FORMS[form]
    return f["d"] ** -0.5 / 8 if f["exact"] else f["d"] ** -0.5


def rows_of(f) -> int:
    return 8 if f["rows"] is None else f["rows"]


# ---- tensors -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=512)
def draw(form, tseed, n):
    """Raw K and V [n, hk, d] of a form's dtype on the CPU from one tensor seed: gaussian (K at scale 2, with scattered exact zeros); the
    exact form's K holds integers in [-7, 7]."""
    f, g = FORMS[form], torch.Generator().manual_seed(tseed)
    shape = (n, f["hk"], f["d"])
    if f["exact"]:
        k = torch.randint(-7, 8, shape, generator=g).float()
    else:
        k = 2.0 * torch.randn(shape, generator=g)
        k[torch.rand(shape, generator=g) < 0.02] = 0
    v = torch.randn(shape, generator=g)
    return k.to(f["dtype"]), v.to(f["dtype"])


@functools.lru_cache(maxsize=512)
def queries(form, qseed, n):
    """Query rows [n, h, d]: gaussian; integers in [-7, 7] in the exact form."""
    f, g = FORMS[form], torch.Generator().manual_seed(qseed)
    shape = (n, f["h"], f["d"])
    q = torch.randint(-7, 8, shape, generator=g).float() if f["exact"] else torch.randn(shape, generator=g)
    return q.to(f["dtype"])


def rule_mask(t, c, dtype, window=None, parents=None):
    """[1, 1, c, t] additive: 0 where query row i of the last c keys' rows sees key j, the dtype's most negative finite value elsewhere.
    Causal: j <= p = i + t - c; with a window also j > p - window; with `parents` (a draft tree over the last c keys) the context
    below t - c and, of the draft, node i and its ancestors."""
    j = torch.arange(t).view(1, t)
    p = torch.arange(c).view(c, 1) + (t - c)
    if parents is None:
        seen = j <= p
        if window is not None:
            seen &= j > p - window
    else:
        seen = (j < t - c).expand(c, t).clone()
        for i in range(c):
            a = i
            while a >= 0:
                seen[i, t - c + a] = True
                a = parents[a]
    return torch.zeros(c, t, dtype=dtype).masked_fill_(~seen, torch.finfo(dtype).min).view(1, 1, c, t)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Seq:
    def __init__(self, keys=(), released=0):
        self.keys, self.released = list(keys), released  # keys: (tensor seed, draw size, row) of every key ever given

    def copy(self):
        return Seq(self.keys, self.released)

    def block(self, i):
        return tuple(self.keys[PAGE * i:PAGE * (i + 1)])


class Model:
    def __init__(self, form):
        self.form, self.f = form, FORMS[form]
        self.live = {}                     # (pool, seq) -> Seq
        self.content = [{}, {}, {}]        # [pool][page] -> the block written there
        self.images = {}                   # name -> (the Seqs, the content of the image's pages, the image's books)

    def of(self, pool):
        return [s for p, s in self.live if p == pool]

    def length(self, pool, seq):
        return len(self.live[pool, seq].keys)

    def raw(self, pool, seq):
        """K and V [1, hk, T, d] the sequence was ever given, CPU tensors of the pool's dtype."""
        keys = self.live[pool, seq].keys
        if not keys:
            z = torch.zeros(1, self.f["hk"], 0, self.f["d"], dtype=self.f["dtype"])
            return z, z.clone()
        drawn = [draw(self.form, ts, n) for ts, n, _ in keys]
        return tuple(torch.stack([kv[i][row] for kv, (_, _, row) in zip(drawn, keys)]).transpose(0, 1).unsqueeze(0).contiguous() for i in (0, 1))

    # what the documented operations do to pages and sequences
    def wrote(self, pt, pool, seq, before):
        """`seq` grew from `before` keys: the blocks from before // 16 on were written - none of them on a page with a second owner."""
        s, row = self.live[pool, seq], pt.table[pt.slot(seq)]
        for i in range(before // PAGE, ceil16(len(s.keys))):
            assert pt._owners[row[i]] == 1, f"a write to block {i} of sequence {seq} lands on page {row[i]} with {pt._owners[row[i]]} owners"
            self.content[pool][row[i]] = s.block(i)

    def appended(self, pt, pool, seq, keys):
        s = self.live[pool, seq]
        before, c = len(s.keys), len(keys)
        if not c:
            return
        if self.f["window"] is not None:  # the docstring's rule
            s.released = max(s.released, min(before + c - self.f["window"] - (rows_of(self.f) - 1), PAGE * (before // PAGE)) // PAGE)
        s.keys += keys
        self.wrote(pt, pool, seq, before)

    def forked(self, pt, pool, parent, child):
        s = self.live[pool, child] = self.live[pool, parent].copy()
        if len(s.keys) % PAGE:
            self.wrote(pt, pool, child, len(s.keys))  # (its open block alone: before // 16 is that block)

    def exported(self, pt, pool, seqs):
        books = pt.export(seqs)
        return [self.live[pool, s].copy() for s in seqs], [self.content[pool][p] for p in books["pages"]], books

    def adopted(self, pt, pool, new, image):
        seqs, content, books = image
        for seq, s, (_, gone, row) in zip(new, seqs, books["seqs"]):
            self.live[pool, seq] = s.copy()
            mine = pt.table[pt.slot(seq)]
            for i in range(gone, len(row)):
                self.content[pool][mine[i]] = content[row[i]]


def check_books(pt, model, pool, what=""):
    """The invariants of the module docstring on one pool's host books."""
    live = model.of(pool)
    assert sorted(pt._slot) == sorted(live), f"{what}: live sequences {sorted(pt._slot)}, the model has {sorted(live)}"
    slots = [pt._slot[s] for s in live]
    assert len(set(slots)) == len(slots) and not set(slots) & set(pt._free_slots) and len(set(pt._free_slots)) == len(pt._free_slots)
    assert sorted(slots + pt._free_slots) == list(range(pt.max_seqs)), f"{what}: slots do not partition into free and live"
    owners = [0] * pt.num_pages
    for seq in live:
        s, x = model.live[pool, seq], pt._slot[seq]
        t = len(s.keys)
        assert pt.lengths[x] == t and pt.pages_of[x] == ceil16(t), f"{what}: sequence {seq}: length {pt.lengths[x]}, {pt.pages_of[x]} pages for {t} keys"
        assert pt.released[x] == s.released <= t // PAGE, f"{what}: sequence {seq} of {t} keys: released {pt.released[x]}, the rule gives {s.released}"
        for i in range(s.released, ceil16(t)):
            page = pt.table[x][i]
            assert 0 <= page < pt.num_pages
            owners[page] += 1
            assert model.content[pool].get(page) == s.block(i), f"{what}: block {i} of sequence {seq} is on page {page}, which holds another block"
        if t % PAGE:
            assert pt._owners[pt.table[x][t // PAGE]] == 1, f"{what}: the open block of sequence {seq} has {pt._owners[pt.table[x][t // PAGE]]} owners"
    assert pt._owners.tolist() == owners, f"{what}: owner counts {pt._owners.tolist()}, the live rows give {owners}"
    assert sorted(pt._free_pages) == [p for p in range(pt.num_pages) if not owners[p]], f"{what}: the free stack is not the pages nobody holds"


def books_of(pt):
    """The host books with every row cut at its entries in use (a rolled-back reservation leaves what it wrote beyond them)."""
    return ([row[:n] for row, n in zip(pt.table, pt.pages_of)], pt.pages_of[:], pt.lengths[:], pt.released[:], pt._free_pages[:], pt._free_slots[:],
            dict(pt._slot), pt._next_seq, pt._owners.tolist())


# ---- PagedKVCache's host side on a PageTable alone -----------------------------------------------------------------------------------
class HostImage:
    def __init__(self, books, signature):
        self.books, self.signature = books, signature

    lengths = property(lambda self: [s[0] for s in self.books["seqs"]])

    def state_dict(self):
        return {"books": self.books, "signature": self.signature}

    @classmethod
    def from_state_dict(cls, d):
        return cls({"pages": list(d["books"]["pages"]), "seqs": [(n, g, list(r)) for n, g, r in d["books"]["seqs"]]}, tuple(d["signature"]))


class HostPool:
    """The calls of PagedKVCache a script makes, as its docstring states their books: no bytes, no device."""

    def __init__(self, pages, slots, room, window=None, rows=None):
        self.pt, self.window, self.max_query_rows = PageTable(pages, slots, room), window, rows

    def alloc(self):
        return self.pt.alloc()

    def free(self, seq):
        self.pt.free(seq)

    def length(self, seq):
        return self.pt.length(seq)

    def append(self, seqs, k, v):
        self._append(list(seqs), [k.shape[2]] * len(k))

    def append_ragged(self, seqs, k, v, counts):
        assert len(k) == sum(counts)
        self._append(list(seqs), list(counts))

    def _append(self, seqs, counts):
        pt, undo = self.pt, []
        slots = pt.slots(seqs)
        if not any(counts):
            return
        if self.window is not None:  # the release comes BEFORE the reservation, and is undone when that is refused
            r = 8 if self.max_query_rows is None else self.max_query_rows
            for seq, x, c in zip(seqs, slots, counts):
                if c:
                    t, first = pt.lengths[x], pt.released[x]
                    freed = pt.release(seq, min(t + c - self.window - (r - 1), PAGE * (t // PAGE)))
                    if pt.released[x] != first:
                        undo.append((seq, first, freed))
        try:
            got, _, _ = pt.reserve(seqs, counts)
        except BaseException:
            for u in reversed(undo):
                pt.unrelease(*u)
            raise
        pt.commit(got, counts)

    def fork(self, seq, n=1):
        return self.fork_many([seq] * n)

    def fork_many(self, parents):
        return self.pt.fork(parents)[0] if parents else []

    def reorder(self, seqs, parent_idx):
        seqs, pt = list(seqs), self.pt
        pt.slots(seqs)
        out, forks, kept = [], [], set()
        for j in parent_idx:
            out.append(None if j in kept else seqs[j])
            if j in kept:
                forks.append(seqs[j])
            kept.add(j)
        dropped = [s for j, s in enumerate(seqs) if j not in kept]
        if not forks and not dropped:
            return out
        snap = pt.snapshot(dropped)
        try:
            for s in dropped:  # parents nobody continues are freed before pages are taken
                pt.free(s)
            children = iter(self.fork_many(forks))
        except BaseException:
            pt.restore(snap)
            raise
        return [next(children) if s is None else s for s in out]

    def _signature(self):
        return (self.window or 0, 8 if self.max_query_rows is None else self.max_query_rows)

    def export(self, seqs, device=None):
        books = self.pt.export(list(seqs))
        return HostImage({"pages": list(range(len(books["pages"]))), "seqs": books["seqs"]}, self._signature())

    def _adopt(self, signature, books):
        if tuple(signature) != self._signature() and any(gone for _, gone, _ in books["seqs"]):
            raise ValueError("a sequence has released pages under another (window, max_query_rows)")
        return self.pt.adopt(books)[0]

    def adopt(self, image):
        return self._adopt(image.signature, image.books)

    swap_in = adopt

    def adopt_from(self, other, seqs):
        return self._adopt(other._signature(), other.pt.export(list(seqs)))

    def swap_out(self, seqs):
        image = self.export(seqs)
        for s in seqs:
            self.pt.free(s)
        return image

    def prefill_rows(self, seq, c):
        """attention_flexible_paged(kernel="prefill") with c query rows on `seq`: the docstring's refusals beyond the window."""
        x = self.pt.slot(seq)
        t = self.pt.lengths[x]
        if self.window is not None and t > self.window:
            if self.max_query_rows is None:
                raise ValueError("the prefill kernel has no window rule on a cache made without max_query_rows")
            if PAGE * self.pt.released[x] > max(0, t - c - self.window + 1):
                raise ValueError("the keys are gone")


POOLS = lambda f: [dict(pages=p, slots=SLOTS + JUNK, window=f["window"]) for p in f["pages"]] + (
    [dict(pages=8, slots=2, window=f["window"] + 16)] if f["window"] is not None else [])
JUNK = 2  # (slots the scrambling's sequences need beside the walk's)


def scramble(form, pool, to=lambda t: t):
    """A pool whose free stack no longer counts up, as test_gpu_kv_swap.scrambled's: sequences of 33, 17, 50 and 41 keys are appended
    in pieces and freed out of order - all of them, so the walk starts from an empty pool - and their ids are spent: the walk's
    sequences are 4, 5, ...  The freed pages hold those sequences' bytes."""
    junk = []
    for i, n in enumerate((33, 17, 50, 41)):
        junk.append(pool.alloc())
        for at in range(0, n, 30):
            k, v = draw(form, 900 + 10 * i + at, min(30, n - at))
            pool.append([junk[-1]], to(k.transpose(0, 1).unsqueeze(0).contiguous()), to(v.transpose(0, 1).unsqueeze(0).contiguous()))
    for i in (0, 2, 3, 1):
        pool.free(junk[i])
    return pool


def host_pools(form):
    """The two pools of a form, scrambled, and on a windowed form a third small one under ANOTHER window (what adopting into it must
    refuse)."""
    f = FORMS[form]
    out = [HostPool(kw["pages"], kw["slots"], f["room"], kw["window"], f["rows"]) for kw in POOLS(f)]
    for pool in out[:2]:
        scramble(form, pool)
    return out


# ---- the executor ------------------------------------------------------------------------------------------------------------------------
def _kv(form, op, n, to):
    k, v = draw(form, op["tseed"], n)
    return to(k), to(v)


def _new(op, got):
    got = list(got)
    if "new" in op:
        assert got == op["new"], f"the ids {got} are not the script's {op['new']}"
    op["new"] = got
    return got


def run(op, pools, model, to=lambda t: t, attend=None, before=lambda: None):
    """One op on `pools` (objects with PagedKVCache's methods), the model kept in step.  to(tensor): a CPU tensor where the pools want it;
    attend(pool index, call): makes an attention call of the script (None: none are made); before(): called before every step that may
    launch.  An op with `raises` must raise that exception - the caller checks what a refusal must leave unchanged."""
    if op.get("raises"):
        try:
            _do(op, pools, model, to, attend, before)
        except EXC[op["raises"]]:
            return
        raise AssertionError(f"not refused with {op['raises']}")
    _do(op, pools, model, to, attend, before)


def _do(op, pools, model, to, attend, before):
    kind, form = op["op"], model.form
    p = op.get("pool")
    pool = pools[p] if p is not None else None
    seqs = op.get("seqs", [])
    before()
    if kind == "alloc":
        model.live[p, _new(op, [pool.alloc()])[0]] = Seq()
    elif kind == "free":
        pool.free(seqs[0])
        del model.live[p, seqs[0]]
    elif kind == "append":
        n = op["n"]
        k, v = _kv(form, op, len(seqs) * n, to)  # [b n, hk, d] -> [b, hk, n, d]
        shape = (len(seqs), n) + tuple(k.shape[1:])
        pool.append(seqs, k.view(shape).transpose(1, 2).contiguous(), v.view(shape).transpose(1, 2).contiguous())
        for b, s in enumerate(seqs):
            model.appended(pool.pt, p, s, [(op["tseed"], len(seqs) * n, b * n + i) for i in range(n)])
    elif kind == "append_ragged":
        counts, total = op["counts"], sum(op["counts"])
        pool.append_ragged(seqs, *_kv(form, op, total, to), counts)
        at = 0
        for s, c in zip(seqs, counts):
            model.appended(pool.pt, p, s, [(op["tseed"], total, at + i) for i in range(c)])
            at += c
    elif kind in ("fork", "fork_many"):
        parents = seqs * op["n"] if kind == "fork" else seqs
        new = _new(op, pool.fork(seqs[0], op["n"]) if kind == "fork" else pool.fork_many(seqs))
        for parent, child in zip(parents, new):
            model.forked(pool.pt, p, parent, child)
    elif kind == "reorder":
        new = _new(op, pool.reorder(seqs, op["idx"]))
        old = {s: model.live.pop((p, s)) for s in seqs}
        for j, s in zip(op["idx"], new):
            if s in old:
                model.live[p, s] = old[s]
        for j, s in zip(op["idx"], new):
            if s not in old:
                model.live[p, seqs[j]] = old[seqs[j]]  # (the parent is live: a fork continues a kept one)
                model.forked(pool.pt, p, seqs[j], s)
    elif kind == "swap_out":
        held = model.exported(pool.pt, p, seqs)
        image = pool.swap_out(seqs)
        if op["file"]:
            image = type(image).from_state_dict(image.state_dict())
        assert image.lengths == [len(s.keys) for s in held[0]]
        for s in seqs:
            del model.live[p, s]
        model.images[op["image"]] = held + (image,)
    elif kind == "swap_in":
        *held, image = model.images[op["image"]]
        model.adopted(pool.pt, p, _new(op, pool.swap_in(image)), held)
        del model.images[op["image"]]
    elif kind == "adopt_from":
        src = op["src"]
        held = model.exported(pools[src].pt, src, seqs)
        model.adopted(pool.pt, p, _new(op, pool.adopt_from(pools[src], seqs)), held)
    elif kind == "export_adopt":  # `pool` is the source, which stays live
        dst = op["dst"]
        held = model.exported(pool.pt, p, seqs)
        image = pool.export(seqs, device="cpu" if op["host"] else None)
        before()
        model.adopted(pools[dst].pt, dst, _new(op, pools[dst].adopt(image)), held)
    elif kind == "spec":  # the docstring's recipe for taking speculated tokens back
        seq, parents, n = seqs[0], op["parents"], len(op["parents"])
        snap, = _new(op, pool.fork(seq))
        model.forked(pool.pt, p, seq, snap)
        before()
        k, v = _kv(form, op, n, to)
        pool.append_ragged([seq], k, v, [n])
        model.appended(pool.pt, p, seq, [(op["tseed"], n, i) for i in range(n)])
        if attend is not None and op["call"]:
            before()
            attend(p, op["call"])
        pool.free(seq)
        del model.live[p, seq]
        if op["accept"]:
            before()
            pool.append_ragged([snap], k[op["accept"]], v[op["accept"]], [len(op["accept"])])
            model.appended(pool.pt, p, snap, [(op["tseed"], n, i) for i in op["accept"]])
    elif kind == "prefill_rows":  # a prefill call of c rows: only ever a refusal
        if attend is None:
            pool.prefill_rows(seqs[0], op["rows"])
        else:
            attend(p, {"pool": p, "entry": "prefill", "seqs": seqs, "rows": op["rows"], "qseed": 1})
    elif kind == "check":
        if attend is not None:
            for call in op["calls"]:
                before()
                attend(call["pool"], call)
    else:
        raise ValueError(kind)


def call_operands(model, call):
    """Per sequence of an attention call with query rows: (q1 [1, h, c, d], K, V [1, hk, T, d], the rule's mask [1, 1, c, T]) on the CPU,
    in the call's order; the call's q is the rows of all q1 one behind the other."""
    form, f, p = model.form, model.f, call["pool"]
    counts = ([len(x) for x in call["parents"]] if "parents" in call else call["counts"] if "counts" in call else
              [call["rows"]] * len(call["seqs"]))
    q, at, out = queries(form, call["qseed"], sum(counts)), 0, []
    window = call.get("window", f["window"])
    for b, (s, c) in enumerate(zip(call["seqs"], counts)):
        if c:
            k, v = model.raw(p, s)
            mask = rule_mask(k.shape[2], c, f["dtype"], window, call["parents"][b] if "parents" in call else None)
            out.append((q[at:at + c].transpose(0, 1).unsqueeze(0).contiguous(), k, v, mask))
        at += c
    return out


# ---- the script --------------------------------------------------------------------------------------------------------------------------
class Script(list):
    dropped = 0


_REFUSED_AS = (("no window rule", "rows"), ("keys are gone", "rows"), ("out of pages", "pages"), ("max_pages_per_seq", "room"),
               ("already freed", "freed"), ("sequence slots", "slots"), ("window", "window"))  # a refusal's words -> its kind


def entries_of(form):
    """The attention entries a form allows: shared prefixes and trees need a cache without a window."""
    return ["paged", "prefill", "decode_ragged", "ragged"] + (["shared", "tree"] if FORMS[form]["window"] is None else [])


def _random_tree(rnd, n):
    return [rnd.randint(-1, i - 1) for i in range(n)]


def _call(rnd, model, p, entry, qseed):
    """One attention call over the live sequences of pool p in a shuffled order, or None when the entry has no sequence to take."""
    f = model.f
    seqs = model.of(p)
    rnd.shuffle(seqs)
    lens = [model.length(p, s) for s in seqs]
    w, most = f["window"], rows_of(f)
    call = {"pool": p, "entry": entry, "qseed": qseed}
    if entry in ("paged", "shared", "windowed", "prefill"):
        if entry == "prefill":
            if w is not None and f["rows"] is None:  # no window rule on the prefill route: it runs while every length <= W
                seqs = [s for s, t in zip(seqs, lens) if t <= w]
            rows = rnd.choice((9, 12, most if w is not None and f["rows"] else 20))
        else:
            rows = rnd.randint(1, 8)
        lens = [model.length(p, s) for s in seqs]
        if not seqs or max(lens) < 1:
            return None
        rows = min(rows, max(lens))
        call.update(seqs=[s for s, t in zip(seqs, lens) if t >= rows], rows=rows)
        if entry == "windowed":
            call["window"] = ORACLE_WINDOW
        return call
    if entry == "tree":
        counts = [min(rnd.choice((0, 1, 5, 8, 12)), t) for t in lens]
        call.update(seqs=seqs, parents=[_random_tree(rnd, c) for c in counts])
    else:
        draws = (0, 1, 3, 8) if entry == "decode_ragged" else (0, 1, 5, 12, most if w is not None and f["rows"] else 20)
        counts = []
        for t in lens:
            c = min(rnd.choice(draws), t)
            if c > 8 and w is not None and f["rows"] is None and t > w:
                c = 8
            counts.append(c)
        call.update(seqs=seqs, counts=counts)
    return call if any(counts) else None


def script(form, seed, steps=STEPS):
    """The ops of one walk, a Script (a list; .dropped counts the draws that found no sequence to act on).  Each step draws a pool and
    a kind - the kinds that ran less than twice and the refusals not yet met first - and performs the op on the generator's own pools
    and model, which is how an op's new ids and a refusal's exception are known.  A pool too full for a draw frees a sequence instead.
    Three things are steered: an image comes back a few steps after it left; the first sequence an image brings back is appended one
    key, forked and swapped out again; on the form with room for it one sequence grows across 256 keys and is then forked."""
    f = FORMS[form]
    rnd = random.Random(f"{form}/{seed}")
    pools, model, ops = host_pools(form), Model(form), Script()
    room, entries = PAGE * f["room"], entries_of(form)
    tseeds = iter(range(100000 * (seed + 1), 100000 * (seed + 2)))
    protected, pending, images, state = set(), [], [], {"long": None, "checks": 0, "image": 0, "filed": False}
    seen = set()  # refusal kinds met
    refusals = REFUSALS if f["window"] is not None else REFUSALS[:3]  # (without a window nothing is ever released: two kinds cannot arise)

    def live(p):
        return model.of(p)

    def emit(op):
        """The op on the generator's own pools: what it creates, or the exception that refuses it, goes into the script."""
        before = [books_of(x.pt) for x in pools]
        try:
            run(op, pools, model)
        except (RuntimeError, KeyError, ValueError) as e:
            assert [books_of(x.pt) for x in pools] == before, f"{op}: a refused op changed the books"
            op["raises"] = type(e).__name__
            op["kind"] = next((name for key, name in _REFUSED_AS if key in str(e)), "other")
            seen.add(op["kind"])
            op.pop("new", None)
        for i, x in enumerate(pools):
            check_books(x.pt, model, i, f"{form}/{seed} op {len(ops)} {op}")
        ops.append(op)
        return "raises" not in op

    def fits(p, s, n):
        return model.length(p, s) + n <= room

    def takes(p, new_seqs, pages):
        """Whether pool p has the slots and the pages for `new_seqs` more sequences on `pages` fresh pages."""
        return len(model.of(p)) + new_seqs <= SLOTS and pages <= pools[p].pt.pages_free

    def make_room(p):
        """A pool too full for the op that was drawn: a sequence leaves instead."""
        mine = [s for s in model.of(p) if (p, s) not in protected]
        return emit({"op": "free", "pool": p, "seqs": [max(mine, key=lambda s: (model.length(p, s), rnd.random()))]}) if mine else None

    def fork_op(op):
        p, open_blocks = op["pool"], sum(1 for s in op["seqs"] * op.get("n", 1) if model.length(op["pool"], s) % PAGE)
        return emit(op) if takes(p, len(op["seqs"]) * op.get("n", 1), open_blocks) else make_room(p)

    def adopt_op(op, src, dst):
        return emit(op) if takes(dst, len(op["seqs"]), len(pools[src].pt.export(op["seqs"])["pages"])) else make_room(dst)

    def check(final=False):
        calls = []
        for p in (0, 1):
            names = entries + (["windowed"] if form in ORACLE_FORMS else []) if final else [entries[(seed + state["checks"] + p) % len(entries)]]
            for e in names:
                c = _call(rnd, model, p, e, next(tseeds))
                if c is not None:
                    calls.append(c)
        state["checks"] += 1
        ops.append({"op": "check", "calls": calls, "final": final})

    def step():
        p = rnd.randrange(2)
        kind = rnd.choices(KINDS + ("refuse",), weights=(8, 5, 14, 14, 6, 5, 5, 7, 0, 6, 5, 6, 9))[0]
        done = [o["op"] for o in ops if "raises" not in o]
        short = [k for k in KINDS if k != "swap_in" and done.count(k) < 2]  # every kind at least twice; every refusal met
        if len(seen & set(refusals)) < len(refusals) and rnd.random() < 0.2:
            kind = "refuse"
        elif short and rnd.random() < 0.6:
            kind = rnd.choice(short)
        if pending and rnd.random() < 0.5:  # what an adopted sequence still has to go through
            what, p, s = pending[0]
            if (p, s) not in model.live:
                pending.clear()
                return step()
            if what == "append1" and fits(p, s, 1) and emit({"op": "append", "pool": p, "seqs": [s], "n": 1, "tseed": next(tseeds)}):
                return pending.pop(0)
            if what == "fork" and takes(p, 1, 1) and emit({"op": "fork", "pool": p, "seqs": [s], "n": 1}):
                return pending.pop(0)
            if what == "swap_out" and swap_out(p, [s], final=True):
                return True
            p = rnd.randrange(2)  # (not now: a random op instead)
        if images and (len(ops) - images[0][1] >= 4 or len(images) > 1):  # an image is held over some steps, then comes back
            name, _, chain = images[0]
            _, _, books = model.images[name][:3]
            dst = [d for d in rnd.sample((0, 1), 2) if takes(d, len(books["seqs"]), len(books["pages"]))]
            if not dst:
                return make_room(rnd.randrange(2))
            dst = dst[0]
            if emit({"op": "swap_in", "pool": dst, "image": name}):
                images.pop(0)
                new = ops[-1]["new"]
                if chain and not pending:
                    protected.add((dst, new[0]))
                    pending.extend([("append1", dst, new[0]), ("fork", dst, new[0]), ("swap_out", dst, new[0])])
                return True
        if state["long"] is not None and rnd.random() < 0.35:  # form A: one sequence grows across 256 keys, then is forked
            lp, ls = state["long"]
            if model.length(lp, ls) <= 256:
                return emit({"op": "append", "pool": lp, "seqs": [ls], "n": 30, "tseed": next(tseeds)})
            if not state.get("forked") and takes(lp, 1, 1):
                state["forked"] = emit({"op": "fork", "pool": lp, "seqs": [ls], "n": 1})
                if state["forked"]:
                    protected.add((lp, ops[-1]["new"][0]))
                return state["forked"]
        mine = [s for s in live(p) if (p, s) not in protected]
        if kind == "alloc":
            return emit({"op": "alloc", "pool": p}) if len(model.of(p)) < SLOTS - 1 else make_room(p)
        if kind == "free":
            return emit({"op": "free", "pool": p, "seqs": [rnd.choice(mine)]}) if len(mine) > 1 else emit({"op": "alloc", "pool": p})
        if kind == "append":
            n = rnd.choice((1, 1, 2, 5, 15, 16, 17, 30))
            some = [s for s in rnd.sample(live(p), min(len(live(p)), rnd.randint(1, 3))) if fits(p, s, n)]
            return emit({"op": "append", "pool": p, "seqs": some, "n": n, "tseed": next(tseeds)}) if some else None
        if kind == "append_ragged":
            some = live(p)
            rnd.shuffle(some)
            counts = [c if fits(p, s, c) else 0 for s, c in ((s, rnd.choice((0, 1, 1, 15, 16, 17, 30))) for s in some)]
            return emit({"op": "append_ragged", "pool": p, "seqs": some, "counts": counts, "tseed": next(tseeds)}) if any(counts) else None
        if kind == "fork":
            return fork_op({"op": "fork", "pool": p, "seqs": [rnd.choice(live(p))], "n": rnd.choice((1, 2, 2))}) if live(p) else None
        if kind == "fork_many":
            if not live(p):
                return None
            a = rnd.choice(live(p))
            return fork_op({"op": "fork_many", "pool": p, "seqs": [a, rnd.choice(live(p)), a][:rnd.randint(2, 3)]})
        if kind == "reorder":
            if len(mine) < 2:
                return None
            some = rnd.sample(mine, min(len(mine), rnd.randint(2, 3)))
            idx = [rnd.randrange(len(some)) for _ in some]
            return emit({"op": "reorder", "pool": p, "seqs": some, "idx": idx})
        if kind == "swap_out":
            if not mine or len(images) > 1:
                return None
            return swap_out(p, rnd.sample(mine, min(len(mine), rnd.randint(1, 2))))
        if kind == "adopt_from":
            src = rnd.randrange(2)
            if not live(src):
                return None
            some = rnd.sample(live(src), min(len(live(src)), rnd.randint(1, 2)))
            return adopt_op({"op": "adopt_from", "pool": p, "src": src, "seqs": some}, src, p)
        if kind == "export_adopt":
            if not live(p):
                return None
            some = rnd.sample(live(p), min(len(live(p)), rnd.randint(1, 2)))
            dst = rnd.randrange(2)
            return adopt_op({"op": "export_adopt", "pool": p, "dst": dst, "seqs": some, "host": rnd.random() < 0.5}, p, dst)
        if kind == "spec":
            n = rnd.choice((3, 6, 8, 12))
            pt = pools[p].pt
            some = [s for s in mine if model.length(p, s) >= 1 and fits(p, s, n)
                    and pt.pages_free >= ceil16(model.length(p, s) + n) - ceil16(model.length(p, s)) + 2]
            if not some or len(model.of(p)) >= SLOTS:
                return None
            s = rnd.choice(some)
            parents = _random_tree(rnd, n) if f["window"] is None else list(range(-1, n - 1))  # (a window takes no tree: a chain)
            leaf, path = rnd.randrange(-1, n), []
            while leaf >= 0:
                path.insert(0, leaf)
                leaf = parents[leaf]
            if f["window"] is None:
                call = {"pool": p, "entry": "tree", "seqs": [s], "parents": [parents], "qseed": next(tseeds)}
            else:
                call = {"pool": p, "entry": "decode_ragged" if n <= 8 else "ragged", "seqs": [s], "counts": [n], "qseed": next(tseeds)}
                if n > 8 and (f["rows"] is None or n > f["rows"]):
                    call = None  # (more rows than the windowed cache takes: the block is appended and taken back unattended)
            return emit({"op": "spec", "pool": p, "seqs": [s], "parents": parents, "accept": path, "tseed": next(tseeds), "call": call})
        return refuse(p)

    def swap_out(p, some, final=False):
        name = f"image{state['image']}"
        ok = emit({"op": "swap_out", "pool": p, "seqs": some, "image": name, "file": not state["filed"]})
        if ok:
            state["image"] += 1
            state["filed"] = True  # one image per script goes through state_dict() / from_state_dict()
            images.append((name, len(ops), not final and not pending))
            if final:
                pending.pop(0)
                protected.discard((p, some[0]))
        return ok

    def refuse(p):
        """A call that must be refused, of a kind not yet met if there is one the pool's state allows."""
        for kind in sorted(refusals, key=lambda k: (k in seen, rnd.random())):
            op = None
            some = live(p)
            if kind == "pages" and some:
                some.sort(key=lambda s: model.length(p, s))
                for i in range(1, len(some) + 1):  # the shortest sequences, as many keys as the longest of them has room for
                    n = 16 * (f["room"] - ceil16(model.length(p, some[i - 1])))
                    need = sum(ceil16(model.length(p, s) + n) - ceil16(model.length(p, s)) for s in some[:i])
                    if n > 0 and need > pools[p].pt.pages_free:
                        op = {"op": "append", "pool": p, "seqs": some[:i], "n": n, "tseed": next(tseeds)}
                        break
            elif kind == "room" and some:
                s = max(some, key=lambda s: model.length(p, s))
                n = room - model.length(p, s) + 1
                if n <= 128:
                    op = {"op": "append", "pool": p, "seqs": [s], "n": n, "tseed": next(tseeds)}
            elif kind == "freed" and pools[p].pt._next_seq > len(pools[p].pt._slot):
                gone = rnd.choice([s for s in range(pools[p].pt._next_seq) if (p, s) not in model.live])
                op = {"op": "append", "pool": p, "seqs": [gone], "n": 1, "tseed": next(tseeds)}
            elif kind == "window" and len(pools) > 2:
                some = [s for s in some if model.live[p, s].released]
                if some:
                    op = {"op": "adopt_from", "pool": 2, "src": p, "seqs": [rnd.choice(some)]}
            elif kind == "rows" and f["window"] is not None:
                for s in some:
                    t, gone = model.length(p, s), model.live[p, s].released
                    c = rows_of(f) + 1
                    while c <= t and not (t > f["window"] and (f["rows"] is None or PAGE * gone > max(0, t - c - f["window"] + 1))):
                        c += 1
                    if gone and c <= t:
                        op = {"op": "prefill_rows", "pool": p, "seqs": [s], "rows": c}
                        break
            if op is not None:
                emit(op)  # (a window's release may make room after all: then it is an append like any other)
                return True
        return None

    emit({"op": "alloc", "pool": 0})
    emit({"op": "alloc", "pool": 1})
    first = ops[0]["new"][0]  # (both pools have handed out the same ids so far)
    emit({"op": "append", "pool": 0, "seqs": [first], "n": 37, "tseed": next(tseeds)})
    if f["room"] > 16:
        state["long"] = (0, first)
        protected.add((0, first))
    emit({"op": "alloc", "pool": 1})  # an empty sequence leaves with the first image: a swap_out at length 0
    emit({"op": "append", "pool": 1, "seqs": [first], "n": 32, "tseed": next(tseeds)})
    swap_out(1, [first, first + 1])
    while len(ops) < steps:
        if len(ops) >= 10 * (state["checks"] + 1) - 1:  # every tenth op
            check()
        elif step() is None:
            ops.dropped += 1
    while images:  # what is still out comes back where there is room
        name, _, _ = images.pop(0)
        books = model.images[name][2]
        for d in (0, 1):
            if takes(d, len(books["seqs"]), len(books["pages"])):
                emit({"op": "swap_in", "pool": d, "image": name})
                break
    check(final=True)
    return ops


def replay(form, ops, on_op=None):
    """The script on fresh HostPools with the books checked after every op: (pools, model).  on_op(i, op, pools, model) after each."""
    pools, model = host_pools(form), Model(form)
    for i, op in enumerate(ops):
        before = [books_of(x.pt) for x in pools]
        try:
            run(dict(op), pools, model)
        except Exception as e:
            raise AssertionError(f"form {form} op {i} {op}: {e}") from e
        if op.get("raises"):
            assert [books_of(x.pt) for x in pools] == before, f"form {form} op {i} {op}: a refused op changed the books"
        for j, x in enumerate(pools):
            check_books(x.pt, model, j, f"form {form} op {i} {op}")
        if on_op is not None:
            on_op(i, op, pools, model)
    return pools, model


# ---- what a script reaches ----------------------------------------------------------------------------------------------------------------
def facts(form, ops):
    """A replay on the host, watched: the op counts by kind, the refusals by kind, and the states the walk is there for."""
    out = {"ops": {}, "refused": {}, "owners3": False, "fork_released": False, "swap_lens": set(), "chain": 0, "reused": False, "ragged": set(),
           "dropped": ops.dropped / len(ops), "entries": set(), "final": set(), "grouped": False}
    stage, ever, closed = {}, [{}, {}, {}], [{}, {}, {}]  # an adopted sequence's stage; [pool][page] -> the holders of its present / last tenure

    def on_op(i, op, pools, model):
        kind, p = op["op"], op.get("pool")
        if op.get("raises"):
            out["refused"][op["kind"]] = out["refused"].get(op["kind"], 0) + 1
        else:
            out["ops"][kind] = out["ops"].get(kind, 0) + 1
        out["owners3"] |= any(int(x.pt._owners.max()) >= 3 for x in pools)
        for j, x in enumerate(pools):  # a page that two sequences held goes back and is taken by another while one of the two lives
            now = {}
            for seq, slot in x.pt._slot.items():
                for page in x.pt.table[slot][x.pt.released[slot]:x.pt.pages_of[slot]]:
                    now.setdefault(page, set()).add(seq)
            for page in range(x.pt.num_pages):
                cur, was = now.get(page, set()), ever[j].get(page, set())
                if was and not cur & was:  # (also inside one op: an append takes what its own release gave back)
                    closed[j][page], was = was, set()
                if cur and not was and len(closed[j].get(page, ())) >= 2 and closed[j][page] & set(x.pt._slot):
                    out["reused"] = True
                ever[j][page] = was | cur
        if op.get("raises"):
            return
        if kind in ("fork", "fork_many", "spec"):
            out["fork_released"] |= any(model.live[p, c].released > 0 for c in op["new"] if (p, c) in model.live)
        for key in [k for k in stage if k not in model.live]:
            if not (kind == "swap_out" and key[0] == p and key[1] in op["seqs"] and stage[key] == 2):
                del stage[key]
        ones = (op["seqs"] if op.get("n") == 1 else []) if kind == "append" else [s for s, c in zip(op["seqs"], op["counts"]) if c == 1] if kind == "append_ragged" else []
        for key in list(stage):
            if key[0] != p:
                continue
            if stage[key] == 0 and key[1] in ones:
                stage[key] = 1
            elif stage[key] == 1 and kind in ("fork", "fork_many") and key[1] in op["seqs"]:
                stage[key] = 2
            elif stage[key] == 2 and kind == "swap_out" and key[1] in op["seqs"]:
                stage[key] = 3
            out["chain"] = max(out["chain"], stage.get(key, 0))
        if kind in ("swap_in", "adopt_from", "export_adopt"):
            stage.update({(op.get("dst", p), s): 0 for s in op["new"]})
        if kind == "swap_out":
            out["swap_lens"] |= {len(x.keys) for x in model.images[op["image"]][0]}
        calls = op["calls"] if kind == "check" else [op["call"]] if kind == "spec" and op["call"] else []
        for call in calls:
            out["entries"].add(call["entry"])
            if kind == "check" and op["final"]:
                out["final"].add(call["entry"])
            if call["entry"] == "ragged":
                out["ragged"] |= {min(c, 9) for c in call["counts"]}
            if call["entry"] == "shared":
                x = pools[call["pool"]].pt
                slots = x.slots(call["seqs"])
                lens = [x.lengths[y] for y in slots]
                out["grouped"] |= any(len(mem) > 1 and keys >= 32 and chunk_of(lens[mem[0]]) == 32 for mem, keys in x.prefix_groups(slots, lens, chunk_of))

    replay(form, ops, on_op)
    return out


def unmet(form, fc):
    """The conditions a script of the GPU file must meet, as a list of those it misses."""
    f, miss = FORMS[form], []
    windowed = f["window"] is not None
    miss += [f"op {k} ran {fc['ops'].get(k, 0)} times" for k in KINDS if fc["ops"].get(k, 0) < 2]
    miss += [f"no refusal of kind {k}" for k in (REFUSALS if windowed else REFUSALS[:3]) if not fc["refused"].get(k)]
    if fc["dropped"] > 0.1:
        miss.append(f"{fc['dropped']:.2f} of the ops were dropped")
    if not fc["owners3"]:
        miss.append("no page with 3 owners")
    if windowed and not fc["fork_released"]:
        miss.append("no fork of a sequence with released pages")
    if windowed and not fc["reused"]:
        miss.append("no freed page taken by another sequence while a former co-owner lives")
    lens = fc["swap_lens"]
    if not (0 in lens and any(n % 16 for n in lens) and any(n and n % 16 == 0 for n in lens)):
        miss.append(f"swap_out at lengths {sorted(lens)}")
    if fc["chain"] < 3:
        miss.append(f"an adopted sequence got to stage {fc['chain']} of append 1 / fork / swap")
    if set(entries_of(form)) - fc["entries"]:
        miss.append(f"entries {sorted(set(entries_of(form)) - fc['entries'])} never called")
    if not {0, 1, 9} <= fc["ragged"]:
        miss.append(f"ragged counts classes {sorted(fc['ragged'])}")
    if form in ORACLE_FORMS and not {"ragged", "windowed", "tree"} <= fc["final"]:
        miss.append(f"final calls {sorted(fc['final'])}")
    if f["room"] > 16 and not fc["grouped"]:
        miss.append("no shared prefix of >= 32 keys grouped at chunk 32")
    return miss


# ---- the rules against the reference ------------------------------------------------------------------------------------------------------
def oracle_calls(ops):
    """The final ragged, windowed and tree calls of a script."""
    return [c for c in ops[-1]["calls"] if c["entry"] in ("ragged", "windowed", "tree")]


def oracle_reference(model, call, acc=torch.float32):
    """_attention.comparator on the model's raw tensors with the call's rule as a mask, sequence by sequence: the rows of O [sum c, h, d]
    in the dtype, the row maxima [sum c, h] fp32 and the row sums [sum c, h] fp64."""
    cfg, outs, maxs, sums = model.f["cfg"], [], [], []
    for q1, k, v, mask in call_operands(model, call):
        o, s2, _ = A.comparator(q1, k, v, scale_of(model.form), mask, cfg, cfg, acc=acc)
        m = s2.float().amax(dim=-1)
        outs.append(o[0].transpose(0, 1))
        maxs.append(m[0].transpose(0, 1))
        sums.append(torch.exp((s2.float() - m[..., None]).double()).sum(-1)[0].transpose(0, 1))
    return torch.cat(outs), torch.cat(maxs), torch.cat(sums)


def spreads(form, ops):
    """The comparator's own spread - fp32 against acc=torch.float64, relative L2 over the whole output - on every oracle call of a script."""
    _, model = replay(form, ops)
    return {(c["pool"], c["entry"]): A._rel(oracle_reference(model, c)[0], oracle_reference(model, c, torch.float64)[0]) for c in oracle_calls(ops)}

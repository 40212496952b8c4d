"""The scheduler walk of tests/_kv_walk.py on the host: its scripts on PageTable alone with the books checked after every op, and the
arithmetic that says the scripts tests/test_gpu_kv_walk.py runs reach what they are there for.  No GPU.

The conditions (unmet()) are asserted per (form, seed) of _kv_walk.SEEDS, which were chosen here, on the CPU, as the first seeds that
meet them: every op kind executes at least twice; a refusal of every kind the form admits (out of pages, beyond max_pages_per_seq, a
freed id - and, on a form with a window, adopting under another window and more query rows than the cache keeps keys for; without a
window nothing is ever released, so those two cannot arise); at most 10 % of the drawn ops dropped for lack of a sequence; a page with
three owners; swap_out at a length that is no multiple of 16, at a multiple of 16 and at 0; an adopted sequence that is then appended
one key, forked and swapped out again; every attention entry called, attention_flexible_paged_ragged with counts 0, 1 and > 8; on a
form with a window a fork of a sequence with released pages, and a page two sequences held that goes back and is taken by another
sequence while one of the two lives (without a window a shared page goes back only with its last owner); on form A a sequence across
256 keys whose fork shares >= 32 keys in one group at chunk 32."""
import collections

import pytest
import torch

import _kv_walk as W
from lqer_amd.kvcache import tree_masks

CASES = [(form, seed) for form in W.FORMS for seed in W.SEEDS[form]]
IDS = [f"{f}-{s}" for f, s in CASES]


@pytest.mark.parametrize("form", list(W.FORMS))
def test_the_books_hold_after_every_op(form):
    """36 scripts per form: script() checks the books after every op it performs and that a refused op leaves them as they were;
    replay() does so again on fresh pools, and must hand out the ids the script names."""
    met = collections.Counter()
    for seed in range(36):
        ops = W.script(form, seed)
        assert 70 <= len(ops) <= 80 and ops[-1]["op"] == "check" and ops[-1]["final"]
        pools, model = W.replay(form, ops)
        assert sorted(model.live) == sorted((p, s) for p, x in enumerate(pools) for s in x.pt._slot)
        met.update(o["kind"] for o in ops if o.get("raises"))
    assert all(met[k] for k in (W.REFUSALS if W.FORMS[form]["window"] is not None else W.REFUSALS[:3])), met


def test_a_script_is_a_function_of_form_and_seed():
    for form, seed in (("A", 1), ("E", 3)):
        assert list(W.script(form, seed)) == list(W.script(form, seed))
    assert list(W.script("B", 0)) != list(W.script("B", 2))


@pytest.mark.parametrize("form, seed", CASES, ids=IDS)
def test_the_gpu_scripts_reach_what_they_are_there_for(form, seed):
    ops = W.script(form, seed)
    fc = W.facts(form, ops)
    print(f"walk {form}/{seed}: {len(ops)} ops, {ops.dropped} dropped; ran {dict(sorted(fc['ops'].items()))}; refused {dict(sorted(fc['refused'].items()))}")
    assert W.unmet(form, fc) == []
    assert 60 <= len(ops) <= 80 and sum(o["op"] == "check" for o in ops) >= 7


@pytest.mark.parametrize("form, seed", [c for c in CASES if c[0] in W.ORACLE_FORMS], ids=[i for c, i in zip(CASES, IDS) if c[0] in W.ORACLE_FORMS])
def test_the_comparators_own_spread_leaves_a_margin_of_ten(form, seed):
    """The final ragged, windowed and tree calls are compared with _attention.comparator at BAR = 1e-3: admissible only where the
    comparator's own spread (fp32 against fp64 products and softmax) is at most 1e-4 on those very inputs."""
    got = W.spreads(form, W.script(form, seed))
    assert {e for _, e in got} == {"ragged", "windowed", "tree"}
    for (pool, entry), spread in sorted(got.items()):
        print(f"own spread {form}/{seed} pool {pool} {entry}: {spread:.2e}")
        assert spread <= 1e-4, f"the comparator's own spread {spread:.2e} leaves no margin of 10 under the bar: another seed"


def test_the_exact_forms_scores_are_exact():
    """Form X: q and K are integers in [-7, 7] and the scaling is a power of two, so a score is at most 64 * 49 steps of one grid -
    exact in fp32 in any order - and the row maximum can be asked for bit for bit."""
    f = W.FORMS["X"]
    k, _ = W.draw("X", 5, 40)
    q = W.queries("X", 6, 9)
    for x in (k, q):
        assert torch.equal(x.float(), x.float().round()) and float(x.abs().max()) == 7
    assert f["d"] * 49 < 2 ** 24 and W.scale_of("X") == 2.0 ** -6


def test_check_books_fails_on_broken_books():
    """The checker has teeth: each of these breaks one invariant by hand."""
    def fresh():
        ops = W.script("B", 0)[:30]
        return W.replay("B", ops)

    def broken(poke, match):
        pools, model = fresh()
        pt = pools[0].pt
        seq = max(pt._slot, key=lambda s: pt.length(s))
        assert pt.length(seq) >= 17
        poke(pt, model, seq, pt._slot[seq])
        with pytest.raises(AssertionError, match=match):
            W.check_books(pt, model, 0)

    def stale_row(pt, model, seq, x):  # the row names a page that holds another block
        pt.table[x][pt.released[x]] = pt._free_pages[-1]

    def reused(pt, model, seq, x):  # a held page is handed out again
        pt._free_pages.append(pt.table[x][pt.pages_of[x] - 1])

    def miscounted(pt, model, seq, x):
        pt._owners[pt.table[x][pt.pages_of[x] - 1]] += 1

    def early(pt, model, seq, x):  # released beyond the rule
        pt.released[x] += 1

    def lost_slot(pt, model, seq, x):
        pt._free_slots.pop()

    broken(stale_row, "holds another block|owner counts")
    broken(reused, "free stack")
    broken(miscounted, "owner")
    broken(early, "released")
    broken(lost_slot, "slots")


def test_the_rule_masks():
    """rule_mask against the rules' words: causal, the window p - W < j <= p, and a tree row's bits as tree_masks gives them."""
    lo = torch.finfo(torch.float16).min
    m = W.rule_mask(10, 3, torch.float16)[0, 0]
    assert [int((r == 0).sum()) for r in m] == [8, 9, 10] and float(m[0, 8]) == lo
    m = W.rule_mask(40, 3, torch.float16, window=20)[0, 0]
    assert [(r == 0).nonzero().flatten().tolist() for r in m] == [list(range(18, 38)), list(range(19, 39)), list(range(20, 40))]
    parents = [-1, 0, 0, 1, -1, 4, 3]
    m = W.rule_mask(19, 7, torch.float16, parents=parents)[0, 0]
    for i, bits in enumerate(tree_masks(parents)):
        assert (m[i, :12] == 0).all() and [j for j in range(7) if float(m[i, 12 + j]) == 0] == [j for j in range(7) if bits >> j & 1]


def test_the_models_window_rule_is_the_docstrings():
    """W = 20, R = 8: an append of c keys to T keys releases the pages wholly below min(T + c - 27, 16 (T // 16))."""
    model = W.Model("B")
    pool = W.HostPool(24, 2, 8, 20, None)
    seq = pool.alloc()
    model.live[0, seq] = W.Seq()
    want = {30: 0, 60: 1, 61: 2, 91: 3, 92: 4}  # 30 + 30 - 27 = 33 -> 16 (30 // 16) = 16; 60 + 1 - 27 = 34; 61 + 30 - 27 = 64 -> 48; 91 + 1 - 27 = 65
    t = 0
    for n in (30, 30, 1, 30, 1):
        k = torch.zeros(1, 2, n, 64)
        pool.append([seq], k, k)
        model.appended(pool.pt, 0, seq, [(1, 200, t + i) for i in range(n)])
        t += n
        assert model.live[0, seq].released == want[t] == pool.pt.released[0], t
        W.check_books(pool.pt, model, 0)

"""Prompt blocks shared by reference in the paged K/V pool, host side: the reference counts of the block allocator, the
prefix plan at block granularity, the scheduler under a fake stepper (random queues with shared prefixes at the smallest pool), the block
accounting of the 16 x 16 queue, the table validation, the refusals and the new entries of the C ABI."""
import os
import random
import re
import subprocess

import pytest
import torch

from tests.test_inflight_host import issue_workload
from tests.test_prefix_host import IMG, _bench_queue
from visualcla import inflight as I
from visualcla import prefix as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vcla_attn_extend_rows_paged", "vcla_llama_extend_rows_paged")
R = 16


# ------------------------------------------------------------------ 1. the allocator's reference counts
def test_a_block_returns_to_the_stack_only_with_its_last_holder():
    a = I.KvBlockAllocator(6)
    x = a.alloc(3)
    assert [a.holders(b) for b in x] == [1, 1, 1] and a.shared == 0 and a.holders(5 if 5 not in x else 0) in (0, 1)
    a.retain(x[:2])
    a.retain(x[:1])
    assert [a.holders(b) for b in x] == [3, 2, 1] and (a.used, a.available, a.shared, a.shared_peak) == (3, 3, 2, 2)
    a.free(x)                                                    # one holder each: only the unshared block goes back
    assert [a.holders(b) for b in x] == [2, 1, 0] and (a.used, a.available, a.shared) == (2, 4, 1)
    y = a.alloc(4)
    assert y is not None and not set(y) & set(x[:2]) and x[2] in y and a.alloc(1) is None and a.peak == 6
    a.free(x[:2])
    assert [a.holders(b) for b in x[:2]] == [1, 0] and a.available == 1 and a.shared == 0
    a.free(x[:1])
    a.free(y)
    assert (a.used, a.available, a.peak, a.shared_peak) == (0, 6, 6, 2)


def test_the_old_errors_still_raise_and_retain_checks_its_blocks():
    a = I.KvBlockAllocator(4)
    x = a.alloc(2)
    a.retain(x)
    a.free(x)
    a.free(x)
    with pytest.raises(ValueError, match="not allocated"):
        a.free(x)                                                # the third free of blocks that had two holders
    y = a.alloc(1)
    for bad in ([7], [-1], y + y, [b for b in range(4) if b not in y][:1]):
        with pytest.raises(ValueError, match="not allocated"):
            a.free(bad)
        with pytest.raises(ValueError, match="KvBlockAllocator.retain: blocks .* are not allocated"):
            a.retain(bad)
    assert a.used == 1 and a.holders(y[0]) == 1 and a.shared == 0      # a refused call changes nothing


# ------------------------------------------------------------------ 2. the plan at block granularity
def _random_queue(rng, n):
    """prompts with shared prefixes: a few heads, a few images, tails of their own; some exact duplicates and strict prefixes"""
    heads = [[rng.randint(3, 50) for _ in range(rng.choice([5, 17, 33, 40]))] for _ in range(3)]
    prompts, keys = [], []
    for i in range(n):
        h = rng.choice(heads)
        if rng.random() < 0.5:
            k = rng.randint(0, 2)
            p = [1] + h + [IMG] * 24 + [rng.randint(3, 50) for _ in range(rng.randint(1, 30))]
        else:
            k = None
            p = [1] + h + [rng.randint(3, 50) for _ in range(rng.randint(1, 50))]
        if prompts and rng.random() < 0.15:
            j = rng.randrange(len(prompts))
            p, k = list(prompts[j]) + [rng.randint(3, 50) for _ in range(rng.choice([0, 0, 9]))], keys[j]
        prompts.append(p)
        keys.append(k)
    return prompts, keys


def test_block_plan_is_the_exact_plan_rounded_down():
    rng = random.Random(3)
    shared = 0
    for case in range(30):
        n, slots = rng.randint(2, 40), rng.choice([2, 4, 8])
        prompts, keys = _random_queue(rng, n)
        ex = P.plan(prompts, keys, IMG, slots)
        pl = P.plan(prompts, keys, IMG, slots, block_rows=R)
        assert pl.block_rows == R and pl.T == ex.T and pl.slots == slots and pl.pool_rows == ex.pool_rows
        for i in range(n):
            assert pl.P[i] % R == 0 and pl.P[i] <= pl.T[i] - 1 and pl.P[i] == ex.P[i] // R * R
            assert pl.source[i] == (ex.source[i] if pl.P[i] else None)
            if pl.P[i]:
                c = pl.source[i]
                assert c < i and prompts[i][:pl.P[i]] == prompts[c][:pl.P[i]] and pl.P[i] <= pl.entries[c].rows
                if IMG in prompts[c][:pl.P[i]]:
                    assert keys[i] == keys[c]                    # the image by value (equal keys stand for equal images)
            if pl.image_from[i] is not None:                     # features come from the creator it reads, the same image
                assert pl.image_from[i] == pl.source[i] and keys[i] == keys[pl.source[i]] and not pl.vision_needed[i]
            has_slot_behind = keys[i] is not None and max(k for k, t in enumerate(prompts[i]) if t == IMG) >= pl.P[i]
            assert (pl.vision_needed[i] or pl.image_from[i] is not None) == has_slot_behind
        assert all(e.rows % R == 0 and e.rows == ex.entries[c].rows // R * R and e.readers == [j for j in ex.entries[c].readers if pl.P[j]]
                   for c, e in pl.entries.items())
        assert pl.vision_runs == ex.vision_runs and pl.peak_pool_rows <= ex.peak_pool_rows
        for members in ([i for i in range(lo, min(lo + slots, n))] for lo in range(0, n, slots)):
            assert [m for ps in P.passes(pl, members) for m in ps] and all(pl.source[i] not in ps or pl.source[i] is None for ps in P.passes(pl, members) for i in ps)
        shared += sum(pl.P)
    assert shared > 2000
    for bad in (0, -16, True, 2.5):
        with pytest.raises(ValueError, match="block_rows must be a positive integer"):
            P.plan([[1, 2]], [None], None, 2, block_rows=bad)


def test_block_plan_of_the_benchmark_queue():
    """16 images x 16 questions, T = 128, the slot ending at row 90: the exact plan reuses 90 rows per reader (11168 rows computed), whole blocks
    reach row 80 -- 16 x 128 + 240 x 48 = 13568 rows computed of 32768, still 16 vision runs: the ten slot rows behind row 80 take the creator's features"""
    prompts, keys = _bench_queue(common_head=False)
    ex = P.plan(prompts, keys, IMG, slots=64)
    pl = P.plan(prompts, keys, IMG, slots=64, block_rows=R)
    assert ex.rows_computed == 11168 and ex.vision_runs == 16
    assert pl.vision_runs == 16 and pl.rows_computed == 16 * 128 + 240 * 48 == 13568 and pl.rows_reused == 32768 - 13568
    assert sorted(pl.entries) == list(range(16)) and all(e.rows == 80 for e in pl.entries.values()) and pl.peak_pool_rows == 16 * 80
    assert [pl.image_from[i] for i in range(16, 256)] == [i % 16 for i in range(16, 256)] and pl.image_from[:16] == [None] * 16
    assert P.passes(pl, list(range(64))) == [list(range(16)), list(range(16, 64))]


# ------------------------------------------------------------------ 3. the scheduler under a fake stepper
def _bound(pl):
    return I.blocks_for(min(pl.pool_rows, pl.peak_pool_rows))


def _smallest_pool(pl, T, budgets):
    """exactly the plan's bound on what entries may hold alone plus the largest single need"""
    return _bound(pl) + max(I.blocks_for(t + b) for t, b in zip(T, budgets))


def test_random_queues_with_shared_prefixes_at_the_smallest_pool():
    rng = random.Random(17)
    waits = cancels = hits = shared_rows = 0
    for case in range(40):
        n, slots, c = rng.randint(2, 30), rng.choice([1, 2, 3, 4, 8]), rng.choice([1, 3, 8])
        prompts, keys = _random_queue(rng, n)
        T = [len(p) for p in prompts]
        budgets = [rng.randint(1, 40) for _ in range(n)]
        pl = P.plan(prompts, keys, IMG, min(slots, n), block_rows=R)
        eos_at = {i: rng.randint(1, budgets[i]) for i in range(n) if rng.random() < 0.25}
        stops = [[[1000 * (i + 1) + 3]] if rng.random() < 0.2 else None for i in range(n)]
        kill = {i for i in range(n) if rng.random() < 0.15}
        pool_blocks = _smallest_pool(pl, T, budgets)
        seen_used = []

        def watch(s):
            assert s.pool.used <= s.pool.n_blocks == pool_blocks                             # held blocks never exceed the pool
            held = {b for bl in s.blocks.values() for b in bl} | {b for bl in s.entry_blocks.values() for b in bl}
            assert s.pool.used == len(held)
            assert sorted(s.blocks) == sorted(i for i in s.slot_req if i is not None)
            for i, bl in s.blocks.items():
                assert len(bl) == I.blocks_for(T[i] + s.budget[i]) and len(set(bl)) == len(bl)
                # no block with two holders lies at or behind a holder's first written row: a reader writes from P_i on; a creator's entry rows lie in
                # front of T_c, where it decodes, and its prefill -- the one pass that writes them -- runs before the pass of any reader (prefix.passes)
                first = pl.P[i] // R
                for idx, b in enumerate(bl):
                    if s.pool.holders(b) > 1:
                        assert idx < first or (i in pl.entries and (idx + 1) * R <= pl.entries[i].rows <= T[i]), (case, i, idx)
            only_entries = held - {b for bl in s.blocks.values() for b in bl}
            assert len(only_entries) <= _bound(pl)
            for c_, bl in s.entry_blocks.items():                # an entry holds its creator's leading blocks, at their logical indices
                assert len(bl) == pl.entries[c_].rows // R and (c_ not in s.blocks or s.blocks[c_][:len(bl)] == bl)
            holders = {}
            for bl in list(s.blocks.values()) + list(s.entry_blocks.values()):
                for b in bl:
                    holders[b] = holders.get(b, 0) + 1
            assert all(s.pool.holders(b) == k for b, k in holders.items())
            seen_used.append(s.pool.used)
        sch, log = I.simulate(budgets, slots, c, eos_at=eos_at, prompt_lens=T, has_image=[k is not None for k in keys], max_position_embeddings=256, stops=stops,
                              on_tokens=lambda i, toks, fin: i in kill, kv_pool_tokens=pool_blocks * R, watch=watch, block_plan=pl)
        res = sch.ordered_results()                              # raises unless every request finished
        assert len(res) == n and sorted(i for _, _, i in log) == list(range(n))
        at = {i: bd for bd, _, i in log}
        assert all(at[i] <= at[i + 1] for i in range(n - 1)), (case, at)                      # nobody overtakes
        assert sch.pool.used == 0 and not sch.blocks and not sch.entry_blocks and sch.pool.available == pool_blocks and sch.pool.shared == 0
        st = sch.stats
        assert st["kv_pool_blocks"] == pool_blocks and max(seen_used) == st["kv_blocks_peak"] <= pool_blocks
        assert st["kv_rows_shared"] == sum(pl.P) and st["kv_blocks_shared_peak"] == sch.pool.shared_peak and sch.decode_from == dict(enumerate(T))
        waits += st["admission_waits_blocks"]
        cancels += st["cancelled"]
        hits += st["stop_hits"]
        shared_rows += st["kv_rows_shared"]
    assert waits > 50 and cancels > 10 and hits > 10 and shared_rows > 2000     # the gate, the cancellations, the stops and the sharing all took part


def test_nothing_alike_is_share_prefix_at_zero_sharing():
    rng = random.Random(23)
    for case in range(15):
        n, slots, c = rng.randint(1, 30), rng.choice([1, 3, 4, 8]), rng.choice([1, 3, 8])
        prompts = [[1, 1000 + i] + [rng.randint(3, 50) for _ in range(rng.randint(1, 60))] for i in range(n)]      # no two prompts share 16 rows
        T = [len(p) for p in prompts]
        budgets = [rng.randint(1, 40) for _ in range(n)]
        eos_at = {i: rng.randint(1, budgets[i]) for i in range(n) if rng.random() < 0.25}
        pl = P.plan(prompts, [None] * n, None, min(slots, n), block_rows=R)
        assert sum(pl.P) == 0 and not pl.entries
        kw = dict(eos_at=eos_at, prompt_lens=T, max_position_embeddings=256)
        ref, ref_log = I.simulate(budgets, slots, c, share_prefix=True, **kw)
        sch, log = I.simulate(budgets, slots, c, kv_pool_tokens=ref.slots * ref.ctx_max, block_plan=pl, **kw)
        assert log == ref_log and sch.decode_from == ref.decode_from and sch.ordered_results() == ref.ordered_results()
        assert {k: v for k, v in sch.stats.items() if k in ref.stats} == ref.stats
        assert sch.stats["admission_waits_blocks"] == sch.stats["kv_rows_shared"] == sch.stats["kv_blocks_shared_peak"] == 0 and sch.pool.used == 0


# ------------------------------------------------------------------ 4. accounting of the 16 x 16 queue
ACCOUNTING = {}          # (slots, share) -> peak blocks, filled by the test below and printed: the numbers of DESIGN.md section 7l


@pytest.mark.parametrize("slots", [64, 256])
def test_accounting_of_the_16x16_queue(slots):
    """the 16 x 16 queue with the budgets of the 7c queue, 64 and 256 slots, an ample pool: the peak with shared blocks against the peak of the
    paged call without (padded admission: every request reserves T + budget rows of its own)"""
    prompts, keys = _bench_queue(common_head=False)
    budgets = issue_workload(0, 256)
    T = [128] * 256
    kw = dict(prompt_lens=T, has_image=[True] * 256, max_position_embeddings=2048)
    plain, _ = I.simulate(budgets, slots, 8, kv_pool_tokens=slots * 640, **kw)
    pl = P.plan(prompts, keys, IMG, slots, block_rows=R)
    sch, _ = I.simulate(budgets, slots, 8, kv_pool_tokens=slots * 640, block_plan=pl, **kw)
    a, b = plain.stats["kv_blocks_peak"], sch.stats["kv_blocks_peak"]
    print(f"[shared blocks] 16 x 16 queue, {slots} slots: peak {a} blocks without share_blocks, {b} with ({sch.stats['kv_blocks_shared_peak']} shared at once, "
          f"{sch.stats['kv_rows_shared']} rows by reference, {sch.stats['admission_groups']} admissions)")
    assert sch.stats["steps"] == plain.stats["steps"] and sch.stats["admission_waits_blocks"] == plain.stats["admission_waits_blocks"] == 0
    assert sch.stats["kv_rows_shared"] == 240 * 80 and sch.pool.used == 0
    assert (a, b, sch.stats["kv_blocks_shared_peak"]) == {64: (1385, 1145, 80), 256: (4241, 3041, 80)}[slots]
    assert b < a


# ------------------------------------------------------------------ 5. the table validation
def test_table_rows_accept_the_sharing_they_should_and_reject_each_violation():
    from visualcla import _lib as L
    kw = dict(n_blocks=12, ld=5)
    # a creator (live, its two leading blocks held by its entry too) and two readers at P = 32, one at P = 16
    t = L.kv_page_rows([[4, 9, 1], [4, 9, 0, 3], [4, 7]], [40, 60, 20], owned={4: 0, 9: 1, 11: -1}, shared=[[4, 9], [4, 9], [4]], **kw)
    assert t.tolist() == [[4, 9, 1, -1, -1], [4, 9, 0, 3, -1], [4, 7, -1, -1, -1]]
    assert torch.equal(L.kv_page_rows([[5, 2, 7], [0]], [40, 16], owned=(6,), shared=[[], []], **kw), L.kv_page_rows([[5, 2, 7], [0]], [40, 16], owned=(6,), **kw))
    for rows, need, owned, shared, why in (
            ([[4, 9, 1], [9, 4, 0]], [40, 40], {}, [[4, 9], [9, 4]], "1: shared block 9 at logical index 0 is held at logical index 1 elsewhere"),
            ([[4, 9, 1], [4, 9, 0]], [40, 40], {}, [[4, 9], [4]], "1: block 9 is owned twice .it is shared elsewhere and this row would write it"),
            ([[4, 9, 1], [4, 1, 0]], [40, 40], {}, [[4], [4, 1]], "1: shared block 1 at logical index 1 is written by another holder"),
            ([[4, 9]], [20], {4: -1}, [[4]], "0: shared block 4 at logical index 0 is written by another holder"),
            ([[4, 9]], [20], {9: 1}, [[4]], "0: block 9 is owned twice"),
            ([[4, 9]], [20], {4: 2}, [[4]], "0: shared block 4 at logical index 0 is held at logical index 2 elsewhere"),
            ([[4, 9]], [20], {}, [[9]], r"0: the shared blocks \[9\] are not the first 1 entries"),
            ([[4, 4]], [20], {}, [[4]], "0: a block stands twice in the row"),
            ([[4, 12]], [20], {}, [[4]], "0: block 12 outside the pool of 12"),
            ([[4]], [20], {}, [[4]], "0: 1 blocks of 16 rows for the 20 rows"),
            ([[0, 1, 2, 3, 4, 5]], [10], {}, [[0]], "0: 6 blocks for a table of 5")):
        with pytest.raises(ValueError, match="kv table row " + why):
            L.kv_page_rows(rows, need, owned=owned, shared=shared, **kw)
    with pytest.raises(ValueError, match="1 shared lists for 2 rows"):
        L.kv_page_rows([[1], [2]], [1, 1], shared=[[]], **kw)


def test_the_scheduler_hands_the_validation_what_it_needs():
    """two requests about one image and a stranger through a real scheduler: the rows the admission pass validates, pass by pass"""
    from visualcla import _lib as L
    prompts = [[1] + [7] * 40 + [20], [1] + [7] * 40 + [21, 22], [1, 9] + [8] * 30]
    pl = P.plan(prompts, [None] * 3, None, 3, block_rows=R)
    assert pl.P == [0, 32, 0] and pl.entries[0].rows == 32
    sch = I.InflightScheduler([len(p) for p in prompts], [4, 4, 4], [False] * 3, 3, 256, kv_pool_tokens=16 * R, block_plan=pl)
    (g,) = sch.admit(sch.free_slots())
    assert g.requests == [0, 1, 2] and g.ragged and sch.blocks[1][:2] == sch.blocks[0][:2] and len(set(sch.blocks[1][2:]) | set(sch.blocks[0]) | set(sch.blocks[2])) == 3 + 1 + 3
    assert P.passes(pl, g.requests) == [[0, 2], [1]]
    rows, need, shared, owned = sch.page_rows([0, 2], pending=[1])
    assert shared == [[], []] and owned == {} and need == [46, 36]
    L.kv_page_rows(rows, need, 16, 16, owned, shared=shared)
    rows, need, shared, owned = sch.page_rows([1])
    assert shared == [sch.blocks[0][:2]] and [owned[b] for b in sch.blocks[0]] == [0, 1, -1] and all(owned[b] == -1 for b in sch.blocks[2])
    L.kv_page_rows(rows, need, 16, 16, owned, shared=shared)
    with pytest.raises(ValueError, match="is owned twice"):      # the same rows without the shared lists: the plain check refuses them
        L.kv_page_rows(rows, need, 16, 16, set(owned))
    assert "entry_blocks" in vars(sch) and sch.entry_blocks == {}           # request 1 was the last planned reader: the entry dropped its hold
    assert [sch.pool.holders(b) for b in sch.blocks[0]] == [2, 2, 1]


# ------------------------------------------------------------------ 6. refusals
def _bare_model():
    from visualcla.modeling_visualcla import VisualCLAModel
    m = VisualCLAModel.__new__(VisualCLAModel)
    m._device = torch.device("cpu")
    m.generation_config = None
    m._ctx = None
    return m


def test_refusals_name_the_argument():
    import visualcla
    m = _bare_model()
    with pytest.raises(ValueError, match=r"^share_blocks=True needs kv_pool_tokens \(it shares blocks of the paged K/V pool"):
        m.generate_many([], share_blocks=True)
    for bad in (1, 0, "yes", 2.5, [True]):
        with pytest.raises(ValueError, match=r"^share_blocks must be a bool \(got " + re.escape(repr(bad))):
            m.generate_many([], kv_pool_tokens=64, share_blocks=bad)
        with pytest.raises(ValueError, match="share_blocks must be a bool"):
            visualcla.chat_many(None, [], kv_pool_tokens=64, share_blocks=bad)
    with pytest.raises(ValueError, match="share_blocks=True needs kv_pool_tokens"):
        visualcla.chat_many(None, [], share_blocks=True)
    assert I.check_share_blocks(None, None) is False and I.check_share_blocks(False, None) is False and I.check_share_blocks(True, 64) is True
    with pytest.raises(ValueError, match=r"generate_many: share_blocks=True with prefix_cache"):
        m.generate_many([], kv_pool_tokens=64, share_blocks=True, prefix_cache=object())
    # the existing refusals keep their text, with or without the new argument
    with pytest.raises(ValueError, match=r"generate_many: kv_pool_tokens with share_prefix=True \(the ragged admission pass needs a paged vcla_attn_extend_rows"):
        m.generate_many([], kv_pool_tokens=64, share_prefix=True, share_blocks=True)
    from visualcla.modeling_visualcla import VisualCLAModel

    class _Unset:
        def __getattr__(self, name):
            return None
    with pytest.raises(ValueError, match=r"cannot be combined with the e4m3 K/V cache .*, share_blocks=True with image_at_head=True, share_blocks=True with an attention_mask "
                                         r"that masks positions \(request 2, 5\)$"):
        VisualCLAModel._refuse_inflight_conflicts(_Unset(), 0, True, 0, None, True, True, [2, 5], "share_blocks=True")
    with pytest.raises(ValueError, match=r"share_prefix=True with image_at_head=True$"):
        VisualCLAModel._refuse_inflight_conflicts(_Unset(), 0, False, 0, None, True, True)
    # the scheduler: a plan without a pool, a plan of another queue, and the up-front refusal with every offender in one message
    pl = P.plan([[1] + [7] * 40 + [20], [1] + [7] * 40 + [21]], [None, None], None, 2, block_rows=R)
    with pytest.raises(ValueError, match="share_blocks=True needs kv_pool_tokens"):
        I.InflightScheduler([42, 42], [4, 4], [False] * 2, 2, 256, block_plan=pl)
    with pytest.raises(ValueError, match="share_blocks=True with image_at_head=True"):
        I.InflightScheduler([42, 42], [4, 4], [False] * 2, 2, 256, image_at_head=True, kv_pool_tokens=256, block_plan=pl)
    with pytest.raises(ValueError, match="the plan must be made at block_rows=16 for the 3 requests"):
        I.InflightScheduler([42, 42, 5], [4, 4, 4], [False] * 3, 2, 256, kv_pool_tokens=256, block_plan=pl)
    with pytest.raises(ValueError, match="the plan must be made at block_rows=16"):
        I.InflightScheduler([42, 42], [4, 4], [False] * 2, 2, 256, kv_pool_tokens=256, block_plan=P.plan([[1, 2], [1, 3]], [None, None], None, 2))
    assert _bound(pl) == 2
    with pytest.raises(ValueError) as e:
        I.InflightScheduler([42, 42], [4, 30], [False] * 2, 2, 256, kv_pool_tokens=4 * R, block_plan=pl)
    assert re.search(r"kv_pool_tokens=64: a pool of 4 blocks of 16 rows cannot hold request 0 \(42 \+ 4 rows = 3 blocks\), 1 \(42 \+ 30 rows = 5 blocks\) "
                     r"beside the 2 blocks shared prefixes may hold \(share_blocks=True\)$", str(e.value)), str(e.value)
    I.InflightScheduler([42, 42], [4, 30], [False] * 2, 2, 256, kv_pool_tokens=7 * R, block_plan=pl)


# ------------------------------------------------------------------ 7. the ABI
def test_new_symbols_are_declared_exported_and_bound(tmp_path):
    from visualcla import _lib as L
    header = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    assert re.search(r"#define\s+VCLA_ABI_VERSION\s+5\b", header)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1], name
    assert len(L.SYMBOLS["vcla_attn_extend_rows_paged"][1]) == len(L.SYMBOLS["vcla_attn_extend_rows"][1]) + 1
    assert len(L.SYMBOLS["vcla_llama_extend_rows_paged"][1]) == len(L.SYMBOLS["vcla_llama_extend_rows"][1]) + 1
    assert lib.vcla_version() == 5
    src = tmp_path / "shared_blocks_abi.c"
    src.write_text('#include "visualcla_hip.h"\n'
                   "int main(void) {\n"
                   "    int (*f)(const void*, void*, void*, const float*, const float*, void*, const vcla_extend_seq*, int, int, int, int, int, int, float, int,\n"
                   "             int, int, void*, size_t, const vcla_kv_pages*, void*) = vcla_attn_extend_rows_paged;\n"
                   "    int (*g)(vcla_ctx*, const void*, const vcla_extend_seq*, int, void*, int, int, float*, void*, size_t, const vcla_kv_pages*, void*) =\n"
                   "        vcla_llama_extend_rows_paged;\n"
                   "    return (f != 0 && g != 0) ? 0 : 1;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "shared_blocks_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

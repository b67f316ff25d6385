"""The paged K/V cache of the slots, host side: the block allocator, the block-gated admission of the scheduler
under a fake stepper, the byte accounting of the 7c queue, the tight-pool queue of the GPU test, the refusals and the new entries of the C ABI."""
import os
import random
import re
import subprocess

import pytest
import torch

from tests import paged_queue as PQ
from tests.test_inflight_host import issue_workload
from visualcla import inflight as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vcla_kv_pool_bytes", "vcla_attn_decode_paged", "vcla_llama_decode_slots_paged")
GIB = 1 << 30


# ------------------------------------------------------------------ 1. the allocator
def test_allocator_alloc_free_peak_and_exhaustion():
    a = I.KvBlockAllocator(10)
    assert (a.n_blocks, a.used, a.peak, a.available) == (10, 0, 0, 10)
    x, y = a.alloc(4), a.alloc(3)
    assert len(set(x) | set(y)) == 7 and all(0 <= b < 10 for b in x + y) and (a.used, a.peak, a.available) == (7, 7, 3)
    assert a.alloc(4) is None and (a.used, a.available) == (7, 3)          # exhaustion takes nothing
    a.free(x)
    assert (a.used, a.peak) == (3, 7)
    z = a.alloc(7)
    assert z is not None and not set(z) & set(y) and (a.used, a.peak) == (10, 10) and a.alloc(1) is None and a.alloc(0) == []
    a.free(y + z)
    assert (a.used, a.peak, a.available) == (0, 10, 10)


def test_allocator_refuses_a_double_free_and_foreign_blocks():
    a = I.KvBlockAllocator(4)
    x = a.alloc(2)
    a.free(x)
    with pytest.raises(ValueError, match="not allocated"):
        a.free(x)
    y = a.alloc(1)
    for bad in ([7], [-1], y + y, [b for b in range(4) if b not in y][:1]):
        with pytest.raises(ValueError, match="not allocated"):
            a.free(bad)
    assert a.used == 1                                           # a refused free takes nothing back
    for bad in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match="n_blocks"):
            I.KvBlockAllocator(bad)


# ------------------------------------------------------------------ 2. the scheduler under a fake stepper
def _largest_need(T, budgets):
    return max(I.blocks_for(t + b) for t, b in zip(T, budgets))


def test_random_queues_at_the_smallest_pool_complete_in_arrival_order():
    rng = random.Random(11)
    waits = cancels = hits = 0
    for case in range(40):
        n, slots, c = rng.randint(1, 30), rng.choice([1, 2, 3, 4, 8]), rng.choice([1, 3, 8])
        T = [rng.randint(1, 90) for _ in range(n)]
        budgets = [rng.randint(1, 40) for _ in range(n)]
        img = [rng.random() < 0.4 for _ in range(n)]
        eos_at = {i: rng.randint(1, budgets[i]) for i in range(n) if rng.random() < 0.25}
        stops = [[[1000 * (i + 1) + 3]] if rng.random() < 0.2 else None for i in range(n)]          # its own third token
        kill = {i for i in range(n) if rng.random() < 0.15}
        pool_blocks = _largest_need(T, budgets)
        seen_used = []

        def watch(s):
            assert s.pool.used <= s.pool.n_blocks == pool_blocks
            assert s.pool.used == sum(len(b) for b in s.blocks.values())
            assert sorted(s.blocks) == sorted(i for i in s.slot_req if i is not None)       # exactly the running requests hold blocks
            assert all(len(s.blocks[i]) == I.blocks_for(s.decode_from[i] + s.budget[i]) for i in s.blocks)
            seen_used.append(s.pool.used)
        sch, log = I.simulate(budgets, slots, c, eos_at=eos_at, prompt_lens=T, has_image=img, max_position_embeddings=256, stops=stops,
                              on_tokens=lambda i, toks, fin: i in kill, kv_pool_tokens=pool_blocks * 16, watch=watch)
        res = sch.ordered_results()                              # raises unless every request finished
        assert len(res) == n and sorted(i for _, _, i in log) == list(range(n))
        at = {i: bd for bd, _, i in log}
        assert all(at[i] <= at[i + 1] for i in range(n - 1)), (case, at)                    # nobody overtakes
        assert sch.pool.used == 0 and not sch.blocks and sch.pool.available == pool_blocks  # the allocator ends empty
        st = sch.stats
        assert st["kv_pool_blocks"] == pool_blocks and max(seen_used) == st["kv_blocks_peak"] <= pool_blocks
        assert 0 < st["kv_rows_reserved_peak"] <= 16 * st["kv_blocks_peak"]
        waits += st["admission_waits_blocks"]
        cancels += st["cancelled"]
        hits += st["stop_hits"]
    assert waits > 50 and cancels > 10 and hits > 10             # the gate, the cancellations and the stops all took part


def test_an_ample_pool_changes_nothing():
    rng = random.Random(5)
    for case in range(20):
        n, slots, c = rng.randint(1, 40), rng.choice([1, 3, 4, 16]), rng.choice([1, 3, 8])
        T = [rng.randint(1, 90) for _ in range(n)]
        budgets = [rng.randint(1, 40) for _ in range(n)]
        img = [rng.random() < 0.4 for _ in range(n)]
        eos_at = {i: rng.randint(1, budgets[i]) for i in range(n) if rng.random() < 0.25}
        kw = dict(eos_at=eos_at, prompt_lens=T, has_image=img, max_position_embeddings=256)
        ref, ref_log = I.simulate(budgets, slots, c, **kw)
        sch, log = I.simulate(budgets, slots, c, kv_pool_tokens=slots * ref.ctx_max, **kw)
        assert log == ref_log and sch.decode_from == ref.decode_from and sch.ordered_results() == ref.ordered_results()
        assert sch.stats["admission_waits_blocks"] == 0 and sch.pool.used == 0
        assert {k: v for k, v in sch.stats.items() if k in ref.stats} == ref.stats          # groups, steps, tokens: all of today's counters


def test_the_head_of_the_queue_waits_and_nobody_overtakes():
    # 3 blocks: request 0 takes 2 (T 20 + 12), request 1 needs 2 and waits although a slot is free and request 2 (1 block) would fit
    sch, log = I.simulate([12, 12, 4], 3, 4, prompt_lens=[20, 20, 4], kv_pool_tokens=48)
    at = {i: bd for bd, _, i in log}
    assert at[0] == 0 and at[1] > 0 and at[2] >= at[1] and sch.stats["admission_waits_blocks"] >= 1
    # a group's T grows when a longer prompt joins, which raises every member's need: 30 + 2 = 2 blocks each instead of 1 + 2
    sch, log = I.simulate([2, 2], 2, 4, prompt_lens=[4, 30], kv_pool_tokens=48)
    assert [bd for bd, _, _ in log] == [0, 1] and sch.stats["admission_waits_blocks"] == 1
    sch, log = I.simulate([2, 2], 2, 4, prompt_lens=[4, 30], kv_pool_tokens=64)
    assert [bd for bd, _, _ in log] == [0, 0] and sch.decode_from == {0: 30, 1: 30}


# ------------------------------------------------------------------ 3. accounting on the 7c queue
ROW_7B = 2 * 32 * 4096 * 2          # bytes of one K/V row at the 7B shape in bf16: K and V, 32 layers, hidden 4096


@pytest.mark.parametrize("slots,long_one,contiguous_gib", [(64, False, 20), (256, False, 80), (64, True, 64), (256, True, 256)])
def test_accounting_of_the_7c_queue(slots, long_one, contiguous_gib):
    budgets = issue_workload(0, 256)
    assert sum(budgets) == 33072
    if long_one:
        budgets = [1900] + budgets                               # ONE long request, at the head: it runs beside a full batch
    T = [128] * len(budgets)
    ctx_max = 2048 if long_one else 640
    sch, _ = I.simulate(budgets, slots, 8, prompt_lens=T, max_position_embeddings=2048, kv_pool_tokens=slots * ctx_max)
    acc = I.kv_accounting(sch, ROW_7B)
    assert sch.ctx_max == ctx_max and sch.stats["admission_waits_blocks"] == 0
    assert acc["kv_bytes_contiguous"] == contiguous_gib * GIB == acc["kv_bytes"]             # the pool of this run is as large as the contiguous cache
    assert acc["kv_bytes_peak"] == sch.stats["kv_blocks_peak"] * 16 * ROW_7B < acc["kv_bytes_contiguous"]
    print(f"[paged] 7c queue{' + one 1900-token budget' if long_one else ''}, {slots} slots: contiguous {contiguous_gib} GiB, paged peak "
          f"{acc['kv_bytes_peak'] / GIB:.2f} GiB ({sch.stats['kv_blocks_peak']} blocks, {sch.stats['kv_rows_reserved_peak']} rows reserved)")


# ------------------------------------------------------------------ 4. the tight-pool queue of the GPU test
@pytest.mark.parametrize("sps", [1, 3, 8])
def test_the_tight_pool_of_the_gpu_test_makes_the_head_wait(sps):
    Q = 8                                                        # cfg_tiny's query tokens
    T = PQ.prompt_lens(Q)
    pool = PQ.tight_pool_tokens(Q)
    assert pool == 16 * _largest_need(T, PQ.BUDGETS)
    sch, log = I.simulate(PQ.BUDGETS, PQ.MAX_BATCH, sps, prompt_lens=T, has_image=PQ.has_image(), max_position_embeddings=256, kv_pool_tokens=pool)
    assert sch.stats["admission_waits_blocks"] > 0 and sch.stats["kv_blocks_peak"] <= sch.stats["kv_pool_blocks"] == pool // 16 and sch.pool.used == 0
    ref, _ = I.simulate(PQ.BUDGETS, PQ.MAX_BATCH, sps, prompt_lens=T, has_image=PQ.has_image(), max_position_embeddings=256)
    assert sch.ordered_results() == ref.ordered_results() and PQ.ample_pool_tokens(Q, ref.ctx_max) >= 4 * pool


# ------------------------------------------------------------------ 5. refusals
def _bare_model():
    from visualcla.modeling_visualcla import VisualCLAModel
    m = VisualCLAModel.__new__(VisualCLAModel)
    m._device = torch.device("cpu")
    m.generation_config = None
    m._ctx = None
    return m


def test_refusals_name_the_argument():
    m = _bare_model()
    for bad in (0, -16, 2.5, "64", True, False):
        with pytest.raises(ValueError, match=r"kv_pool_tokens must be None or a positive integer \(got " + re.escape(repr(bad))):
            m.generate_many([], kv_pool_tokens=bad)
        with pytest.raises(ValueError, match="kv_pool_tokens must be None or a positive integer"):
            I.InflightScheduler([4], [4], [False], 2, 64, kv_pool_tokens=bad)
    assert I.check_kv_pool_tokens(None) is None and I.check_kv_pool_tokens(1) == 1 and I.check_kv_pool_tokens(16) == 1 and I.check_kv_pool_tokens(17) == 2
    with pytest.raises(ValueError, match=r"generate_many: kv_pool_tokens with share_prefix=True \(the ragged admission pass needs a paged vcla_attn_extend_rows"):
        m.generate_many([], kv_pool_tokens=64, share_prefix=True)
    with pytest.raises(ValueError, match=r"generate_many: kv_pool_tokens with prefix_cache .*paged prefill"):
        m.generate_many([], kv_pool_tokens=64, share_prefix=True, prefix_cache=object())
    with pytest.raises(ValueError, match="kv_pool_tokens with share_prefix=True"):
        I.InflightScheduler([4], [4], [False], 2, 64, share_prefix=True, kv_pool_tokens=64)
    # a request that alone needs more than the pool: every one of them in ONE message, before anything runs
    with pytest.raises(ValueError) as e:
        I.InflightScheduler([10, 40, 20, 5], [6, 30, 45, 5], [False] * 4, 2, 256, kv_pool_tokens=64)
    msg = str(e.value)
    assert re.search(r"kv_pool_tokens=64: a pool of 4 blocks of 16 rows cannot hold request 1 \(40 \+ 30 rows = 5 blocks\), 2 \(20 \+ 45 rows = 5 blocks\)$", msg), msg
    I.InflightScheduler([10, 40, 20, 5], [6, 30, 45, 5], [False] * 4, 2, 256, kv_pool_tokens=80)


def test_chat_many_checks_the_argument_before_anything_else():
    import visualcla
    with pytest.raises(ValueError, match="kv_pool_tokens must be None or a positive integer"):
        visualcla.chat_many(None, [], kv_pool_tokens=0)


def test_table_rows_are_validated_before_the_upload():
    from visualcla import _lib as L
    t = L.kv_page_rows([[5, 2, 7], [0]], [40, 16], n_blocks=8, ld=4)
    assert t.dtype == torch.int32 and t.tolist() == [[5, 2, 7, -1], [0, -1, -1, -1]]
    for rows, need, owned, why in (([[5, 8]], [20], (), "block 8 outside the pool of 8"), ([[5, -1]], [20], (), "block -1 outside the pool"),
                                   ([[5, 2], [2]], [20, 4], (), "1: block 2 is owned twice"), ([[5, 5]], [20], (), "block 5 is owned twice"),
                                   ([[5]], [10], (5,), "block 5 is owned twice"), ([[5, 2]], [33], (), "2 blocks of 16 rows for the 33 rows"),
                                   ([[0, 1, 2, 3, 4]], [70], (), "5 blocks for a table of 4")):
        with pytest.raises(ValueError, match="kv table row .*" + why):
            L.kv_page_rows(rows, need, n_blocks=8, ld=4, owned=owned)


# ------------------------------------------------------------------ 6. the ABI
def test_new_symbols_are_declared_exported_and_bound(tmp_path):
    from visualcla import _lib as L
    header = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    assert re.search(r"#define\s+VCLA_ABI_VERSION\s+5\b", header)
    assert int(re.search(r"#define\s+VCLA_KV_BLOCK_ROWS\s+(\d+)\b", header).group(1)) == L.KV_BLOCK_ROWS == I.KV_BLOCK_ROWS == 16
    assert re.search(r"typedef\s+struct\s+vcla_kv_pages\s*\{\s*const\s+int32_t\s*\*\s*table\s*;[^}]*\bint\s+ld\s*;[^}]*\bint\s+n_blocks\s*;[^}]*\}\s*vcla_kv_pages\s*;", header)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1], name
    assert len(L.SYMBOLS["vcla_llama_decode_slots_paged"][1]) == len(L.SYMBOLS["vcla_llama_decode_slots_stops"][1]) + 1
    assert len(L.SYMBOLS["vcla_attn_decode_paged"][1]) == len(L.SYMBOLS["vcla_attn_decode_rows"][1]) + 1
    assert lib.vcla_version() == 5
    assert (L.KvPages.table.offset, L.KvPages.ld.offset, L.KvPages.n_blocks.offset) == (0, 8, 12)
    assert lib.vcla_kv_pool_bytes(None, 4) == 0
    # the header still compiles as C99 with the new struct, warnings as errors
    src = tmp_path / "paged_abi.c"
    src.write_text('#include "visualcla_hip.h"\n'
                   "int main(void) {\n"
                   "    vcla_kv_pages p = {0, 40, 64};\n"
                   "    int (*f)(const void*, void*, void*, const float*, const float*, void*, int, int, int, int, const int32_t*, const vcla_kv_pages*,\n"
                   "             const int32_t*, int64_t, float, int, int, void*) = vcla_attn_decode_paged;\n"
                   "    size_t (*g)(const vcla_ctx*, int) = vcla_kv_pool_bytes;\n"
                   "    return (f != 0 && g != 0 && p.ld * VCLA_KV_BLOCK_ROWS == 640 && p.n_blocks == 64 && p.table == 0) ? 0 : 1;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "paged_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

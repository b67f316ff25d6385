"""Prefix sharing, host side (visualcla/prefix.py): the plan on hand-written and random queues, the scheduler in share
mode driven by the fake stepper, the derived row accounting of the benchmark-shaped queue, and the refusals that need no GPU."""
import random

import pytest

from visualcla import inflight as I
from visualcla import prefix as P

IMG, IMG_S, IMG_E = 900, 901, 902          # <img_token>, <img>, </img>


def _slot(q=8):
    return [IMG_S] + [IMG] * q + [IMG_E]


def _common(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def _match(prompts, keys, i, c):
    """match(i, c) of the module header, written out independently: ids, then the image rule"""
    m = _common(prompts[i], prompts[c])
    if IMG in prompts[c]:
        f = prompts[c].index(IMG)
        if keys[i] != keys[c]:
            m = min(m, f)
    return m


def _check_properties(prompts, keys, slots, pl):
    n = len(prompts)
    for i in range(n):
        T = len(prompts[i])
        assert 0 <= pl.P[i] <= T - 1
        s = pl.source[i]
        if s is None:
            assert pl.P[i] == 0
        else:
            e = pl.entries[s]
            assert s < i, "a reader before its creator"
            assert pl.min_shared_rows <= pl.P[i] <= min(_match(prompts, keys, i, s), e.rows)          # a common prefix under the image rule, inside the entry
            assert pl.P[i] == min(_match(prompts, keys, i, s), e.rows, T - 1)
            assert i in e.readers and e.last_reader == max(e.readers) >= i
            # the longest usable match among the entries that exist, the oldest on ties
            for c, o in pl.entries.items():
                if c < i:
                    u = min(_match(prompts, keys, i, c), o.rows, T - 1)
                    assert u < pl.P[i] or (u == pl.P[i] and c >= s), (i, s, c)
        has_slot = IMG in prompts[i]
        if keys[i] is None:
            assert not pl.vision_needed[i]
        else:
            last = max(k for k, t in enumerate(prompts[i]) if t == IMG) if has_slot else None
            assert pl.vision_needed[i] == (not (has_slot and last < pl.P[i]))
    for c, e in pl.entries.items():
        assert e.creator == c and 1 <= e.rows <= len(prompts[c]) and e.readers
    for i in range(n):
        rows = sum(e.rows for e in pl.entries.values() if e.creator <= i <= e.last_reader + slots - 1)
        assert rows == pl.live_rows_at(i) <= pl.pool_rows, (i, rows, pl.pool_rows)
    assert pl.rows_reused + pl.rows_computed == sum(len(p) for p in prompts)
    # a request that shares nothing with an existing entry and was not denied its own: nobody before it offers min_shared_rows
    for i in range(n):
        if pl.source[i] is None:
            for c in pl.entries:
                if c < i:
                    assert min(_match(prompts, keys, i, c), pl.entries[c].rows, len(prompts[i]) - 1) < pl.min_shared_rows


# ------------------------------------------------------------------ 1. the plan on hand-written lists
def test_two_images_three_questions_and_a_text_request():
    head = [1] + list(range(10, 30))                               # 21 common rows
    q = [[100 + 10 * k + j for j in range(9)] for k in range(6)]
    A, B = "A", "B"
    _slot = lambda: globals()["_slot"](24)                         # noqa: E731  (26 rows: enough for an entry of its own behind the common head)
    prompts = [head + _slot() + q[0],                              # 0: image A, creates rows [0, 47)
               head + _slot() + q[1],                              # 1: image B: reads the head from 0 (21 rows: up to the first <img_token> = 22), creates
               head + [7] * 12,                                    # 2: text only: reads 21 rows of 0
               head + _slot() + q[2],                              # 3: image A
               head + _slot() + q[3],                              # 4: image B
               head + _slot() + q[4],                              # 5: image A
               head + _slot() + q[5]]                              # 6: image B
    keys = [A, B, None, A, B, A, B]
    pl = P.plan(prompts, keys, IMG, slots=4)
    _check_properties(prompts, keys, 4, pl)
    assert pl.P == [0, 22, 21, 47, 47, 47, 47]                     # <img> itself is a shared id: the match of another image stops at the first <img_token>
    assert pl.source == [None, 0, 0, 0, 1, 0, 1]
    assert pl.vision_needed == [True, True, False, False, False, False, False]
    assert pl.entries[0].rows == 47 and pl.entries[1].rows == 47 and sorted(pl.entries) == [0, 1]
    assert pl.entries[0].last_reader == 5 and pl.entries[1].last_reader == 6
    assert pl.vision_runs == 2 and pl.rows_reused == 22 + 21 + 4 * 47
    # boundary 0 of 4 slots: 0 alone, then its readers 1, 2, 3; the next boundary finds both entries made
    assert P.passes(pl, [0, 1, 2, 3]) == [[0], [1, 2, 3]]
    assert P.passes(pl, [4, 5, 6]) == [[4, 5, 6]]
    assert P.passes(pl, [1, 2, 3, 4]) == [[1, 2, 3], [4]]          # 1's entry is made by this boundary: its reader 4 waits one pass


def test_strict_prefix_equal_ids_other_image_short_match_and_release():
    base = [1] + list(range(10, 40))                               # 31 ids
    prompts = [base,                                               # 0
               base + [50, 51, 52],                                # 1: 0 is a strict prefix of it
               base,                                               # 2: the same prompt again: capped at T - 1
               [1] + list(range(10, 20)) + [99] * 30,              # 3: 11 common rows: below min_shared_rows
               [1, 2, 3] + _slot() + [60, 61, 62, 63, 64, 65, 66, 67],      # 4: image X
               [1, 2, 3] + _slot() + [60, 61, 62, 63, 64, 65, 66, 67]]      # 5: the ids of 4 with image Y
    keys = [None, None, None, None, "X", "Y"]
    pl = P.plan(prompts, keys, IMG, slots=2)
    _check_properties(prompts, keys, 2, pl)
    assert pl.P[:4] == [0, 31, 30, 0] and pl.source[:4] == [None, 0, 0, None]
    assert pl.entries[0].rows == 31 and pl.entries[0].last_reader == 2
    assert pl.P[5] == 0 and pl.source[5] is None                   # the match stops at the first <img_token> (4 rows: below the threshold)
    assert pl.vision_needed == [False] * 4 + [True, True]
    # with the same image the whole prompt but its last row is shared, and the vision stack is skipped
    pl2 = P.plan(prompts, keys[:5] + ["X"], IMG, slots=2)
    assert pl2.P[5] == len(prompts[5]) - 1 and pl2.source[5] == 4 and not pl2.vision_needed[5]
    # a lower threshold admits the short match
    pl3 = P.plan(prompts, keys, IMG, slots=2, min_shared_rows=8)
    assert pl3.P[3] == 11 and pl3.source[3] == 0
    # release: the entry is live from its creator to its last reader (+ slots - 1 arrivals), not before and not after
    assert [pl.live_rows_at(i) for i in range(6)] == [31, 31, 31, 31, 0, 0]


def test_pool_of_one_entry_refuses_nobody():
    a = [1] + list(range(10, 40))
    b = [1] + list(range(50, 80))
    prompts = [a + [5], b + [5], a + [6], b + [6], a + [7], b + [7], b + [8], b + [9]]
    keys = [None] * 8
    free = P.plan(prompts, keys, None, slots=2, pool_rows=1000)
    assert sorted(free.entries) == [0, 1] and free.P == [0, 0, 31, 31, 31, 31, 31, 31] and free.denied == []
    one = P.plan(prompts, keys, None, slots=2, pool_rows=31)
    _check_properties(prompts, keys, 2, one)
    # entry 0 lives until request 4 and slots - 1 = 1 arrival longer: the creators 1, 3 and 5 find the pool full; 6, behind the release, creates for 7
    assert sorted(one.entries) == [0, 6] and one.denied == [1, 3, 5]
    assert one.P == [0, 0, 31, 0, 31, 0, 0, 31] and one.source == [None, None, 0, None, 0, None, None, 6]
    assert one.peak_pool_rows == 31
    none = P.plan(prompts, keys, None, slots=2, pool_rows=0)
    assert none.entries == {} and none.P == [0] * 8 and none.rows_computed == sum(len(p) for p in prompts)
    # the default pool: 16 entries of the longest planned prefix
    assert P.plan(prompts, keys, None, slots=2).pool_rows == 16 * 31


def test_plan_properties_on_random_queues():
    rng = random.Random(5)
    shared = created = denied = image_cut = 0
    for case in range(300):
        n = rng.randint(1, 40)
        slots = rng.choice([1, 2, 4, 8, 64])
        heads = [[1] + [rng.randint(3, 60) for _ in range(rng.choice([4, 18, 25, 40]))] for _ in range(rng.randint(1, 4))]
        images = ["a", "b", "c"][:rng.randint(1, 3)]
        prompts, keys = [], []
        for _ in range(n):
            h = rng.choice(heads)
            if rng.random() < 0.15:
                h = h[:rng.randint(1, len(h))]
            if rng.random() < 0.6:
                k = rng.choice(images)
                body = _slot(rng.choice([4, 8])) if rng.random() < 0.9 else []
            else:
                k, body = None, []
            tail = [rng.randint(3, 12) for _ in range(rng.randint(1, 25))]
            prompts.append(h + body + tail)
            keys.append(k)
        pool = rng.choice([0, 30, 64, 200, 100000, None])
        msr = rng.choice([1, 8, 16])
        pl = P.plan(prompts, keys, IMG, slots, pool_rows=pool, min_shared_rows=msr)
        _check_properties(prompts, keys, slots, pl)
        shared += sum(p > 0 for p in pl.P)
        created += len(pl.entries)
        denied += len(pl.denied)
        image_cut += sum(1 for i, s in enumerate(pl.source) if s is not None and keys[i] != keys[s])
        # passes: every admission window of the queue, in arrival order
        for lo in range(0, n, slots):
            adm = list(range(lo, min(n, lo + slots)))
            ps = P.passes(pl, adm)
            assert sorted(i for p_ in ps for i in p_) == adm
            where = {i: k for k, p_ in enumerate(ps) for i in p_}
            for i in adm:
                s = pl.source[i]
                assert where[i] == (where[s] + 1 if s in where else 0)       # behind its creator's pass, or in the first
        # the pool as generate_many runs it: admissions of 1 .. slots requests in arrival order, prefilled in passes; rows taken from a free
        # list of the plan's peak when an entry is made, given back after its last reader's pass -- it never runs dry, nobody reads a missing entry
        free, held, lo = pl.peak_pool_rows, {}, 0
        assert free <= pl.pool_rows
        while lo < n:
            adm = list(range(lo, min(n, lo + rng.randint(1, slots))))
            lo = adm[-1] + 1
            for members in P.passes(pl, adm):
                for i in members:
                    assert pl.source[i] is None or held[pl.source[i]] >= pl.P[i]
                for i in members:
                    if i in pl.entries:
                        held[i] = pl.entries[i].rows
                        free -= held[i]
                        assert free >= 0, (case, i)
                for i in members:
                    s_ = pl.source[i]
                    if s_ is not None and pl.entries[s_].last_reader == i:
                        free += held.pop(s_)
        assert not held and free == pl.peak_pool_rows
    assert shared > 1000 and created > 300 and denied > 50 and image_cut > 50


# ------------------------------------------------------------------ 2. the scheduler in share mode
def test_share_mode_keeps_results_and_admission_order():
    rng = random.Random(17)
    for case in range(40):
        B = rng.choice([1, 2, 3, 8, 16])
        c = rng.choice([1, 2, 3, 8, 13])
        N = rng.randint(1, 70)
        budgets = [rng.choice([1, 2, rng.randint(1, 60), rng.randint(1, 300)]) for _ in range(N)]
        eos_at = {i: rng.randint(1, budgets[i]) for i in range(N) if rng.random() < 0.3}
        T = [rng.randint(4, 200) for _ in range(N)]
        img = [rng.random() < 0.5 for _ in range(N)]
        a, log_a = I.simulate(budgets, B, c, eos_at=eos_at, prompt_lens=T, has_image=img)
        b, log_b = I.simulate(budgets, B, c, eos_at=eos_at, prompt_lens=T, has_image=img, share_prefix=True)
        # every request into the same slot at the same boundary (the log lists an admission group by group: compare it sorted)
        assert sorted(log_a) == sorted(log_b) and a.ordered_results() == b.ordered_results()
        assert [i for _, _, i in log_b] == sorted(i for _, _, i in log_b)   # ... and one ragged group per admission keeps arrival order
        assert a.stats["steps"] == b.stats["steps"] and a.stats["tokens"] == b.stats["tokens"]
        assert [b.decode_from[i] for i in range(N)] == T                    # nobody is padded
        assert all(a.decode_from[i] >= T[i] for i in range(N))
        assert b.stats["admission_groups"] <= a.stats["admission_groups"]   # one ragged group per admission
    from tests.test_inflight_host import issue_workload
    n = issue_workload(0)
    a, log_a = I.simulate(n, 64, 8)
    b, log_b = I.simulate(n, 64, 8, share_prefix=True)
    assert sorted(log_a) == sorted(log_b) and b.stats["steps"] == a.stats["steps"] == 920 and a.ordered_results() == b.ordered_results()


def test_ragged_groups_ignore_the_three_rules():
    T = [10, 12, 10, 30, 12]
    img = [True, True, False, True, False]
    sch = I.InflightScheduler(T, [5] * 5, img, 8, 2048, share_prefix=True)
    gs = sch.admit(sch.free_slots())
    assert len(gs) == 1 and gs[0].ragged and gs[0].requests == [0, 1, 2, 3, 4] and gs[0].slots == [0, 1, 2, 3, 4]
    assert [sch.decode_from[i] for i in range(5)] == T
    assert all(T[i] + sch.budget[i] <= sch.ctx_max for i in range(5))


# ------------------------------------------------------------------ 3. row accounting of the benchmark-shaped queue, derived
def _bench_queue(common_head: bool):
    """16 images x 16 questions, arrival interleaved by image; prompts as bench.py lays them out: BOS + 23 ids + <img> + 64 <img_token> + </img> + 38
    ids = 128 rows, first <img_token> at row 25, slot ending at row 90"""
    rng = random.Random(9)
    heads = [[rng.randint(3, 800) for _ in range(23)] for _ in range(16)]
    if common_head:
        heads = [heads[0]] * 16
    else:
        for k in range(16):
            heads[k][0] = 3 + k                                    # the one common row is BOS
    prompts, keys = [], []
    for q in range(16):
        for k in range(16):
            tail = [rng.randint(3, 800) for _ in range(38)]
            tail[0] = 3 + q * 16 + k                               # no two questions begin alike
            prompts.append([1] + heads[k] + [IMG_S] + [IMG] * 64 + [IMG_E] + tail)
            keys.append(k)
    assert all(len(p) == 128 and p.index(IMG) == 25 and p[89] == IMG_E for p in prompts)
    return prompts, keys


def test_row_accounting_of_the_benchmark_queue():
    prompts, keys = _bench_queue(common_head=False)
    pl = P.plan(prompts, keys, IMG, slots=64, pool_rows=16 * 90)
    assert P.plan(prompts, keys, IMG, slots=64).pool_rows == 16 * 90           # the default is that pool
    assert pl.vision_runs == 16 and pl.rows_computed == 16 * 128 + 240 * 38 == 11168 and pl.rows_reused == 256 * 128 - 11168
    assert sorted(pl.entries) == list(range(16)) and all(e.rows == 90 for e in pl.entries.values()) and pl.peak_pool_rows == 16 * 90
    # boundary 0: the 16 creators in pass 1, their 48 readers in pass 2
    ps = P.passes(pl, list(range(64)))
    assert ps == [list(range(16)), list(range(16, 64))]
    # (b) a system prompt: the 15 later creators reuse rows [0, 25) of the first entry and still run their vision stack
    prompts_b, keys_b = _bench_queue(common_head=True)
    pb = P.plan(prompts_b, keys_b, IMG, slots=64, pool_rows=16 * 90)
    assert pb.P[:16] == [0] + [25] * 15 and pb.source[:16] == [None] + [0] * 15
    assert pb.rows_computed == 128 + 15 * 103 + 240 * 38 == 10793 and pb.vision_runs == 16
    assert P.passes(pb, list(range(64))) == [[0], list(range(1, 16)) + list(range(16, 64, 16)), [i for i in range(16, 64) if i % 16]]
    # (c) a pool of ONE entry: only image 0's questions share, nobody is refused
    pc = P.plan(prompts, keys, IMG, slots=64, pool_rows=90)
    assert sorted(pc.entries) == [0] and pc.denied[:15] == list(range(1, 16)) and all(keys[c] != 0 for c in pc.denied)
    assert pc.rows_computed == 128 + 15 * 38 + 240 * 128 and pc.vision_runs == 1 + 240
    assert len(pc.P) == 256 and all(p in (0, 90) for p in pc.P)
    _check_properties(prompts, keys, 64, pl)
    _check_properties(prompts_b, keys_b, 64, pb)
    _check_properties(prompts, keys, 64, pc)


# ------------------------------------------------------------------ 4. refusals, no GPU
def test_share_prefix_refusals_are_named_beside_the_old_ones():
    from tests.test_inflight_host import _gc
    from visualcla.modeling_visualcla import VisualCLAModel
    with pytest.raises(ValueError) as e:
        VisualCLAModel._refuse_inflight_conflicts(_gc(num_beams=3, max_time=1.0), kv_fp8=True, share_prefix=True, image_at_head=True, masked_requests=[2, 5])
    msg = str(e.value)
    for word in ("generate_many", "num_beams=3", "max_time", "e4m3", "image_at_head=True", "attention_mask", "request 2, 5"):
        assert word in msg, word
    # without the switch neither is a conflict; with it, an unmasked queue without image_at_head passes
    VisualCLAModel._refuse_inflight_conflicts(_gc(), image_at_head=True, masked_requests=[1])
    VisualCLAModel._refuse_inflight_conflicts(_gc(), share_prefix=True)
    with pytest.raises(ValueError, match="image_at_head"):
        VisualCLAModel._refuse_inflight_conflicts(_gc(), share_prefix=True, image_at_head=True)
    with pytest.raises(ValueError, match="attention_mask"):
        VisualCLAModel._refuse_inflight_conflicts(_gc(), share_prefix=True, masked_requests=[0])


def test_generate_many_and_chat_many_take_the_switch():
    import inspect
    import visualcla
    sig = inspect.signature(visualcla.VisualCLAModel.generate_many)
    assert sig.parameters["share_prefix"].default is False and sig.parameters["prefix_pool_tokens"].default is None
    assert inspect.signature(visualcla.chat_many).parameters["share_prefix"].default is False

"""In-flight batching, host side (visualcla/inflight.py): the scheduler driven by a fake stepper, the derived step bound, the pure-Python
model of the slot step, the refusals of generate_many that need no GPU, and the new entries of the C ABI."""
import os
import random
import re

import numpy as np
import pytest

from visualcla import inflight as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def issue_workload(seed=0, n=256):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(np.exp(rng.normal(np.log(96), 0.8, n))), 8, 512).astype(int).tolist()


# ------------------------------------------------------------------ 1. scheduler + fake stepper
def _check_run(budgets, slots, c, eos_at=None, **kw):
    sch, log = I.simulate(budgets, slots, c, eos_at=eos_at, **kw)
    n = len(budgets)
    res = sch.ordered_results()                                  # raises unless every request finished
    assert sorted(i for _, _, i in log) == list(range(n))        # admitted exactly once
    for i, toks in enumerate(res):
        want = min(budgets[i], (eos_at or {}).get(i, 1 << 30))
        assert len(toks) == want, (i, len(toks), want)
        body = toks[:-1] if (eos_at or {}).get(i) == want else toks
        assert body == [1000 * (i + 1) + k for k in range(1, len(body) + 1)], i     # its own tokens, in order: no slot held two requests
        if (eos_at or {}).get(i) == want:
            assert toks[-1] == 0
    assert sch.stats["tokens"] == sum(len(t) for t in res)
    assert sch.stats["steps"] <= I.step_bound([len(t) for t in res], sch.slots, c) + 1e-9
    return sch, log


def test_every_request_finishes_once_in_request_order():
    rng = random.Random(3)
    budgets = [rng.randint(1, 40) for _ in range(37)]
    eos_at = {i: rng.randint(1, budgets[i]) for i in range(0, 37, 3)}
    sch, log = _check_run(budgets, 4, 3, eos_at)
    assert sch.stats["requests"] == 37 and sch.stats["slots"] == 4
    assert 0 < sch.stats["slot_steps_active"] <= sch.stats["slot_steps_total"] == sch.stats["steps"] * 4


def test_freed_slot_is_refilled_at_the_next_boundary():
    budgets = [9, 2, 30, 30, 5, 5, 5]
    sch, log = _check_run(budgets, 4, 4)
    by_req = {i: (bd, b) for bd, b, i in log}
    assert [by_req[i][0] for i in range(4)] == [0, 0, 0, 0]
    # request 1 (2 tokens: one step) frees slot 1 inside chunk 0 -> request 4 takes it at boundary 1; request 0 (8 steps) ends in chunk 1 -> boundary 2
    assert by_req[4] == (1, 1) and by_req[5] == (2, 0) and by_req[6] == (2, 1)


def test_first_token_that_ends_a_request_never_holds_a_slot():
    budgets = [1, 1, 1, 6, 1, 1]
    sch, log = _check_run(budgets, 2, 8, eos_at={3: 1})
    assert sch.stats["steps"] == 0 and all(bd == 0 for bd, _, _ in log)          # nothing ever needed a decode step


def test_groups_split_by_the_three_rules_only():
    # image / text separate; equal prompts share; different lengths share too (left padding) unless image_at_head
    T = [10, 12, 10, 30, 12]
    img = [True, True, False, True, False]
    sch = I.InflightScheduler(T, [5] * 5, img, 8, 2048)
    gs = sch.admit(sch.free_slots())
    assert [(g.requests, g.image, g.T) for g in gs] == [([0, 1, 3], True, 30), ([2, 4], False, 12)]
    sch = I.InflightScheduler(T, [5] * 5, img, 8, 2048, image_at_head=True)
    gs = sch.admit(sch.free_slots())
    assert [(g.requests, g.T) for g in gs] == [([0], 10), ([1], 12), ([2, 4], 12), ([3], 30)]
    # third rule: T_group + budget_i <= ctx_max for every member.  ctx_max = round_up_64(100 + 60) = 192 capped at 160
    sch = I.InflightScheduler([100, 20, 20], [60, 100, 30], [False] * 3, 8, 160)
    assert sch.ctx_max == 160 and sch.budget == [60, 100, 30]
    gs = sch.admit(sch.free_slots())
    assert [(g.requests, g.T) for g in gs] == [([0, 2], 100), ([1], 20)]         # 100 + 100 > 160: request 1 keeps its budget in a group of its own
    assert all(g.T + sch.budget[i] <= sch.ctx_max for g in gs for i in g.requests)


def test_capacity_and_clipping():
    sch = I.InflightScheduler([30, 50], [20, 500], [False, False], 4, 256)
    assert sch.budget == [20, 206] and sch.ctx_max == 256 and sch.cap == 206
    sch = I.InflightScheduler([30, 50], [20, 40], [False, False], 4, 2048)
    assert sch.ctx_max == 128
    with pytest.raises(ValueError, match="request 2"):
        I.InflightScheduler([30, 50, 256], [20, 40, 5], [False] * 3, 4, 256)


# ------------------------------------------------------------------ 2. the step bound, derived
def test_issue_workload_step_counts():
    n = issue_workload(0)
    assert round(float(np.mean(n))) == 129 and max(n) == 512
    sch, _ = _check_run(n, 64, 8)
    assert sch.stats["steps"] == 920
    assert round(I.step_bound(n, 64, 8)) == 1065
    assert I.static_batch_steps(n, 64) == 1856
    assert -(-sum(x - 1 for x in n) // 64) == 513
    for seed, static, inflight in ((1, 2015, 760), (2, 2037, 872)):
        m = issue_workload(seed)
        assert I.static_batch_steps(m, 64) == static and I.simulate(m, 64, 8)[0].stats["steps"] == inflight


def test_step_bound_on_random_queues():
    rng = random.Random(17)
    for case in range(50):
        kind = case % 5
        B = rng.choice([1, 2, 3, 8, 16])
        c = rng.choice([1, 2, 3, 8, 13])
        N = 0 if kind == 0 else rng.randint(1, B - 1) if (kind == 1 and B > 1) else rng.randint(1, 70)
        budgets = [1] * N if kind == 2 else [rng.choice([1, 2, rng.randint(1, 60), rng.randint(1, 300)]) for _ in range(N)]
        eos_at = {i: rng.randint(1, budgets[i]) for i in range(N) if rng.random() < 0.3}
        sch, _ = _check_run(budgets, B, c, eos_at)
        if N == 0 or kind == 2:
            assert sch.stats["steps"] == 0


# ------------------------------------------------------------------ 3. the host model of the slot step
def test_slot_step_model():
    row_pos, count, budget, cur = [10, -1, 7, 3], [1, 5, 2, 4], [3, 9, 9, 5], [0, 0, 0, 0]
    hist = [[0] * 4 for _ in range(6)]
    hl = [1, -1, 2, 4]
    n = I.slot_step_model([50, 51, 2, 53], row_pos, count, budget, hist, cur, [2, 3], hl)
    # slot 0 continues; slot 1 inactive: untouched; slot 2 meets an eos; slot 3 reaches its budget
    assert n == 1 and row_pos == [11, -1, -1, -1] and count == [2, 5, 3, 5] and cur == [50, 0, 2, 53] and hl == [2, -1, -1, -1]
    assert hist[1][0] == 50 and hist[2][2] == 2 and hist[4][3] == 53 and hist[5][1] == 0
    n = I.slot_step_model([60, 61, 62, 63], row_pos, count, budget, hist, cur, [2, 3], hl)
    assert n == 0 and row_pos == [-1] * 4 and count == [3, 5, 3, 5] and hist[2][0] == 60          # slot 0 hits its budget of 3


# ------------------------------------------------------------------ 4. refusals, no GPU
def _gc(**kw):
    from transformers import GenerationConfig
    from visualcla.modeling_visualcla import _HF_GLOBAL_GENERATION_DEFAULTS
    gc = GenerationConfig(**kw)
    for k, v in _HF_GLOBAL_GENERATION_DEFAULTS.items():
        if getattr(gc, k, None) is None:
            setattr(gc, k, v)
    return gc


@pytest.mark.parametrize("kw, extra, word", [
    (dict(num_beams=2), {}, "num_beams"),
    (dict(do_sample=True, num_return_sequences=3, top_k=5), {}, "num_return_sequences"),
    (dict(prompt_lookup_num_tokens=3), {}, "prompt_lookup_num_tokens"),
    (dict(max_time=2.0), {}, "max_time"),
    (dict(min_length=30, eos_token_id=2), {}, "min_length"),
    (dict(bad_words_ids=[[5]]), {}, "bad_words_ids"),
    (dict(suppress_tokens=[4]), {}, "suppress_tokens"),
    (dict(do_sample=True, typical_p=0.5, top_k=5), {}, "typical_p"),
    (dict(do_sample=True, top_k=0), {}, "top_k"),
    (dict(do_sample=True, top_k=300), {}, "top_k"),
    (dict(min_new_tokens=3, eos_token_id=[2, 3, 4, 5, 6]), {}, "eos_token_id"),
    (dict(eos_token_id=list(range(2, 12))), {}, "eos_token_id"),
    (dict(repetition_penalty=1.1), dict(vocab_size=60000), "vocab_size"),
    (dict(no_repeat_ngram_size=3), dict(max_budget=5000), "max_new_tokens"),
    ({}, dict(kv_fp8=True), "e4m3"),
    (dict(penalty_alpha=0.5), {}, "penalty_alpha"),
])
def test_refusal_matrix(kw, extra, word):
    from visualcla.modeling_visualcla import VisualCLAModel
    with pytest.raises(ValueError, match=word):
        VisualCLAModel._refuse_inflight_conflicts(_gc(**kw), **extra)


def test_refusals_are_all_named_and_supported_configs_pass():
    from visualcla.modeling_utils import DEFAULT_GENERATION_CONFIG
    from visualcla.modeling_visualcla import VisualCLAModel
    with pytest.raises(ValueError) as e:
        VisualCLAModel._refuse_inflight_conflicts(_gc(num_beams=3, max_time=1.0, prompt_lookup_num_tokens=2, bad_words_ids=[[1]]), kv_fp8=True)
    for word in ("generate_many", "num_beams=3", "max_time", "prompt_lookup_num_tokens", "bad_words_ids", "e4m3"):
        assert word in str(e.value)
    with pytest.raises(ValueError, match="not_a_field"):
        VisualCLAModel._refuse_inflight_conflicts(_gc(), leftover_kwargs={"not_a_field": 1})
    for ok in (_gc(), _gc(do_sample=False, eos_token_id=2), _gc(do_sample=True, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=3, min_new_tokens=4,
                                                               eos_token_id=2), _gc(min_length=30), _gc(**{k: v for k, v in DEFAULT_GENERATION_CONFIG.to_dict().items()
                                                                                                          if v is not None and not k.startswith("_") and
                                                                                                          k != "transformers_version"})):
        VisualCLAModel._refuse_inflight_conflicts(ok, vocab_size=49958, max_budget=512)


# ------------------------------------------------------------------ 5. the C ABI
NEW = ("vcla_attn_decode_rows", "vcla_sample_rows", "vcla_slot_step", "vcla_llama_decode_slots")


def test_new_entries_declared_bound_and_exported():
    from visualcla import _lib
    hdr = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    declared = set(re.findall(r"\b(vcla_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "vcla_slot_args" not in declared and "typedef struct vcla_slot_args" in hdr
    assert lib.vcla_version() == 5
    # the ctypes mirror of vcla_slot_args: 3 ints + the eos array, then seven pointers
    assert _lib.SlotArgs.row_pos.offset == 4 * (3 + _lib.SLOT_MAX_EOS) + 4 and _lib.SLOT_MAX_EOS == int(re.search(r"#define VCLA_SLOT_MAX_EOS (\d+)", hdr).group(1))


def test_chat_many_is_exported():
    import visualcla
    assert callable(visualcla.chat_many) and "chat_many" in visualcla.__all__
    assert callable(visualcla.VisualCLAModel.generate_many)

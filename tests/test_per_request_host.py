"""Per-request generation configs and seeds in generate_many, host side: request parsing, the merged refusal,
the host model of the per-row eos lookup, the builder of the sampler's record table, the ABI.  No GPU."""
import ctypes as C
import os
import random
import re

import pytest
import torch

from visualcla import inflight as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gc(**kw):
    from transformers import GenerationConfig
    from visualcla.modeling_visualcla import _HF_GLOBAL_GENERATION_DEFAULTS
    gc = GenerationConfig(**kw)
    for k, v in _HF_GLOBAL_GENERATION_DEFAULTS.items():
        if getattr(gc, k, None) is None:
            setattr(gc, k, v)
    return gc


def _bare_model():
    """a VisualCLAModel without weights or device: what request parsing and config resolution touch"""
    from visualcla.modeling_visualcla import VisualCLAModel
    m = VisualCLAModel.__new__(VisualCLAModel)
    m._device = torch.device("cpu")
    m.generation_config = None
    m._ctx = None
    return m


# ------------------------------------------------------------------ 1. request parsing
def test_request_keys_and_config_resolution():
    from transformers import GenerationConfig
    m = _bare_model()
    ids = torch.arange(3, 9)
    queue = m._resolve_generation_config(None, dict(do_sample=False, max_new_tokens=7, eos_token_id=None))
    raw = [dict(input_ids=ids),
           dict(input_ids=ids, generation_config=GenerationConfig(do_sample=True, top_k=5, temperature=0.7, max_new_tokens=3), seed=11),
           dict(input_ids=ids, generation_config=dict(repetition_penalty=1.3)),
           dict(input_ids=ids, generation_config=dict(repetition_penalty=1.3), max_new_tokens=2),
           dict(input_ids=ids, generation_config=dict(max_new_tokens=5), seed=4)]
    reqs = [m._inflight_request(i, r) for i, r in enumerate(raw)]
    assert [r["seed"] for r in reqs] == [None, 11, None, None, 4]
    gcs, cls, reps = m._request_configs(queue, reqs)
    assert cls == [0, 1, 2, 2, 3] and len(reps) == 4 and gcs[0] is queue and gcs[2] is gcs[3]
    # a GenerationConfig replaces the queue's and is resolved like generate()'s argument (transformers' defaults for what it leaves unset)
    assert gcs[1].do_sample is True and gcs[1].top_k == 5 and gcs[1].temperature == 0.7 and gcs[1].repetition_penalty == 1.0
    # a dict is laid over the queue's resolved config: everything else, an eos the queue switched off included, stays
    assert gcs[2].repetition_penalty == 1.3 and gcs[2].do_sample is False and gcs[2].eos_token_id is None and gcs[2].max_new_tokens == 7
    assert queue.repetition_penalty == 1.0                       # the queue's own config is not written to
    # budget precedence: the request's key, then its config's budget, then the queue's
    assert m._request_budgets(queue, reqs, gcs, [6] * 5) == [7, 3, 7, 2, 5]
    # a request config without a budget of its own falls back to the queue's, not to the library default of 20
    r = m._inflight_request(0, dict(input_ids=ids, generation_config=GenerationConfig(do_sample=True, top_k=5)))
    g1, _, _ = m._request_configs(queue, [r])
    assert m._request_budgets(queue, [r], g1, [6]) == [7]


@pytest.mark.parametrize("bad, word", [
    (dict(session=1), r"request 2: unknown keys \['session'\]"),
    (dict(generation_config=3), "request 2: generation_config must be"),
    (dict(generation_config=dict(tempratur=0.5)), r"request 2: generation_config has fields.*tempratur"),
    (dict(seed=1.5), "request 2: seed must be an integer"),
    (dict(seed=True), "request 2: seed must be an integer"),
])
def test_bad_request_keys_are_refused_by_index(bad, word):
    m = _bare_model()
    queue = m._resolve_generation_config(None, {})
    with pytest.raises(ValueError, match=word):
        ok = m._inflight_request(0, dict(input_ids=torch.arange(3, 9)))
        m._request_configs(queue, [ok, ok, m._inflight_request(2, dict(input_ids=torch.arange(3, 9), **bad))])


# ------------------------------------------------------------------ 2. refusals
def _members(n, special):
    """request index -> config class: class 0 is the rest of the queue, class k + 1 holds special[k]"""
    return [[i for i in range(n) if i not in special]] + [[i] for i in special]


def test_per_request_refusals_are_merged_into_one_message():
    from visualcla.modeling_visualcla import VisualCLAModel
    configs = [_gc(), _gc(num_beams=2), _gc(do_sample=True, typical_p=0.5, top_k=5)]
    with pytest.raises(ValueError) as e:
        VisualCLAModel._refuse_per_request_conflicts(configs, _members(10, [3, 7]), [8] * 10, vocab_size=100)
    msg = str(e.value)
    assert msg.startswith("generate_many (in-flight batching) cannot be combined with ")
    assert "request 3: num_beams=2" in msg and "request 7: typical_p=0.5" in msg and "request 0" not in msg
    # the same reason for several requests under different configs: one entry, all indices
    with pytest.raises(ValueError, match="request 3, 7: num_beams=2"):
        VisualCLAModel._refuse_per_request_conflicts([_gc(), _gc(num_beams=2), _gc(num_beams=2, repetition_penalty=1.0)], _members(10, [3, 7]), [8] * 10)
    # features generate() itself refuses come through by request too
    with pytest.raises(ValueError, match="request 1: .*penalty_alpha"):
        VisualCLAModel._refuse_per_request_conflicts([_gc(), _gc(penalty_alpha=0.5)], _members(3, [1]), [8] * 3)
    # nothing to refuse
    VisualCLAModel._refuse_per_request_conflicts([_gc(), _gc(do_sample=True, top_k=40, top_p=0.9, temperature=0.5, repetition_penalty=1.1,
                                                             no_repeat_ngram_size=15)], _members(4, [2]), [512] * 4, vocab_size=49958)


def test_sampler_limits_apply_to_sampler_rows_only():
    from visualcla import _lib
    from visualcla.modeling_visualcla import VisualCLAModel
    big = _lib.SAMPLE_MAX_HIST + 100
    greedy, sampled = _gc(), _gc(do_sample=True, top_k=5)
    # request 0 greedy with a budget beyond the sampler's history, request 1 sampled with a small one: accepted
    VisualCLAModel._refuse_per_request_conflicts([greedy, sampled], [[0], [1]], [big, 16], vocab_size=100)
    # the other way round: the sampled request's own budget is what counts
    with pytest.raises(ValueError, match=rf"request 1: max_new_tokens={big}"):
        VisualCLAModel._refuse_per_request_conflicts([greedy, sampled], [[0], [1]], [16, big], vocab_size=100)
    # the vocabulary limit is the sampler's: it names the requests that use it, and an all-greedy queue with different eos ids passes
    with pytest.raises(ValueError, match=r"request 1: vocab_size=60000") as e:
        VisualCLAModel._refuse_per_request_conflicts([greedy, sampled], [[0], [1]], [16, 16], vocab_size=60000)
    assert "request 0" not in str(e.value)
    VisualCLAModel._refuse_per_request_conflicts([greedy, _gc(eos_token_id=5)], [[0], [1]], [big, big], vocab_size=60000)


def test_per_queue_refusals_stay_per_queue():
    from visualcla.modeling_visualcla import VisualCLAModel
    configs, members = [_gc(), _gc(repetition_penalty=1.2)], [[0, 2], [1]]
    with pytest.raises(ValueError) as e:
        VisualCLAModel._refuse_per_request_conflicts(configs, members, [8] * 3, kv_fp8=True)
    assert "e4m3" in str(e.value) and "request" not in str(e.value)
    with pytest.raises(ValueError, match="share_prefix=True with image_at_head=True"):
        VisualCLAModel._refuse_per_request_conflicts(configs, members, [8] * 3, share_prefix=True, image_at_head=True)
    with pytest.raises(ValueError, match=r"share_prefix=True with an attention_mask that masks positions \(request 2\)"):
        VisualCLAModel._refuse_per_request_conflicts(configs, members, [8] * 3, share_prefix=True, masked_requests=[2])
    # the existing function and its messages, unchanged
    with pytest.raises(ValueError, match=r"^generate_many \(in-flight batching\) cannot be combined with num_beams=2, the e4m3 K/V cache"):
        VisualCLAModel._refuse_inflight_conflicts(_gc(num_beams=2), kv_fp8=True)


# ------------------------------------------------------------------ 3. the host model of the per-row eos lookup
def _state(B, rng):
    row_pos = [rng.choice([-1, rng.randrange(0, 50)]) for _ in range(B)]
    count = [rng.randrange(0, 5) for _ in range(B)]
    budget = [c + rng.randrange(1, 6) for c in count]
    return row_pos, count, budget, [0] * B, [[0] * B for _ in range(12)], [c if p >= 0 else -1 for c, p in zip(count, row_pos)]


def test_slot_step_model_eos_rows():
    rng = random.Random(3)
    for B in (1, 4, 9):
        ids = [rng.randrange(0, 6) for _ in range(B)]
        a, b = _state(B, random.Random(B)), _state(B, random.Random(B))
        na = I.slot_step_model(ids, a[0], a[1], a[2], a[4], a[3], [2, 3], a[5])
        nb = I.slot_step_model(ids, b[0], b[1], b[2], b[4], b[3], [], b[5], eos_rows=[[2, 3]] * B)
        assert na == nb and a == b                               # all rows share a list: the positional form
    # only the rows whose own list holds the id finish
    row_pos, count, budget, cur = [5, 5, 5, -1], [1, 1, 1, 1], [9, 9, 9, 9], [0] * 4
    hist, hl = [[0] * 4 for _ in range(4)], [1, 1, 1, -1]
    n = I.slot_step_model([7, 7, 8, 7], row_pos, count, budget, hist, cur, [7, 8], hl, eos_rows=[[7], [8], [], [7]])
    assert n == 2 and row_pos == [-1, 6, 6, -1] and count == [2, 2, 2, 1] and hl == [-1, 2, 2, -1] and cur == [7, 7, 8, 0]


# ------------------------------------------------------------------ 4. the record table of the sampler
def test_sample_row_table_round_trip():
    from visualcla import _lib
    rows = [dict(repetition_penalty=1.1, no_repeat_ngram_size=15, min_new_tokens=4, eos_ids=(2, 9), temperature=0.5, top_k=40, top_p=0.9,
                 min_tokens_to_keep=2),
            dict(greedy=True),
            dict(top_k=256, top_p=1.0, temperature=2.0, eos_ids=(1, 2, 3, 4), min_new_tokens=1)]
    arr = _lib.sample_row_table(rows)
    assert C.sizeof(_lib.SampleRow) == 64 and len(arr) == 3
    r = arr[0]
    assert (r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens, r.n_eos, list(r.eos_ids)) == (C.c_float(1.1).value, 15, 4, 2, [2, 9, -1, -1])
    assert (r.temperature, r.top_k, r.use_top_p, r.min_tokens_to_keep, r.greedy, list(r.reserved)) == (0.5, 40, 1, 2, 0, [0, 0])
    assert r.top_p_complement == C.c_float(1.0 - 0.9).value      # the double difference rounded to fp32, as vcla_sample computes it
    r = arr[1]
    assert (r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens, r.n_eos, r.temperature, r.top_k, r.use_top_p, r.min_tokens_to_keep,
            r.greedy) == (1.0, 0, 0, 0, 1.0, 1, 0, 1, 1)
    assert (arr[2].top_k, arr[2].use_top_p, arr[2].top_p_complement, arr[2].n_eos, list(arr[2].eos_ids)) == (256, 0, 0.0, 4, [1, 2, 3, 4])
    # the bytes that are uploaded are the records, in order
    raw = _lib.sample_row_bytes(arr)
    assert raw.shape == (3, 64) and raw.dtype == torch.uint8
    back = (_lib.SampleRow * 3).from_buffer_copy(bytes(raw.numpy().tobytes()))
    assert back[0].top_k == 40 and back[1].greedy == 1 and list(back[2].eos_ids) == [1, 2, 3, 4]
    # the header's record has the same fields in the same order
    hdr = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    body = re.search(r"typedef struct vcla_sample_row \{(.*?)\} vcla_sample_row;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[[^\]]*\])?\s*;", body)
    assert names == [f[0] for f in _lib.SampleRow._fields_]
    eos = _lib.slot_eos_rows([[], [5], list(range(8))])
    assert eos.dtype == torch.int32 and eos.tolist() == [[-1] * 8, [5] + [-1] * 7, list(range(8))]


@pytest.mark.parametrize("kw, word", [
    (dict(top_k=0), "top_k=0"),
    (dict(top_k=257), "top_k=257"),
    (dict(temperature=0.0), "temperature=0"),
    (dict(temperature=-1.0), "temperature=-1"),
    (dict(top_p=0.0), "top_p=0"),
    (dict(top_p=1.5), "top_p=1.5"),
    (dict(eos_ids=(1, 2, 3, 4, 5)), "n_eos=5"),
    (dict(repetition_penalty=0.0), "repetition_penalty=0"),
    (dict(min_tokens_to_keep=0), "min_tokens_to_keep=0"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size=-1"),
    (dict(top_q=1), "unknown fields"),
])
def test_sample_row_table_refuses_out_of_range_records(kw, word):
    from visualcla import _lib
    with pytest.raises(ValueError, match=r"sample row 1: .*" + re.escape(word)):
        _lib.sample_row_table([dict(), kw])
    with pytest.raises(ValueError, match="at most 8 eos ids"):
        _lib.slot_eos_rows([list(range(9))])


# ------------------------------------------------------------------ 5. the C ABI
NEW = ("vcla_sample_rows_table", "vcla_slot_step_rows", "vcla_llama_decode_slots_rows")


def test_new_entries_declared_bound_and_exported():
    from visualcla import _lib
    hdr = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    declared = set(re.findall(r"\b(vcla_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "vcla_sample_row" not in declared and "typedef struct vcla_sample_row" in hdr
    assert lib.vcla_version() == 5


def test_chat_many_takes_per_item_lists():
    import inspect
    import visualcla
    p = inspect.signature(visualcla.chat_many).parameters
    assert p["generation_configs"].default is None and p["seeds"].default is None
    assert "generation_config" in inspect.signature(visualcla.VisualCLAModel.generate).parameters
    assert "seed" not in inspect.signature(visualcla.VisualCLAModel.generate).parameters      # the one-slot route uses a private hook
    with pytest.raises(ValueError, match="seeds has 1 entries for 2 items"):
        visualcla.chat_many(None, [(None, "a"), (None, "b")], seeds=[1])

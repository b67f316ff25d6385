"""The prefix cache that outlives the call, on the MI355X: vcla_kv_blocks_copy bit for bit against torch indexing,
generate_many(share_prefix=True, prefix_cache=) over several calls against the CPU oracle and against the lookup / combination rules
written out on lists, a cache too small for its traffic, the one-slot route, graph and eager, per-request configs, chat_many, a context
rebuild, the refusals, and bf16 at the engine widths on rows a previous call left in the cache."""
import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 16


def _lib():
    from visualcla import _lib as L
    return L


# ------------------------------------------------------------------ 1. the kernel, bitwise
LAYERS, HEADS, SLOTS, CTX, BLOCKS = 2, 3, 3, 48, 5
TABLES = {
    0: [],
    1: [(3, 1, 16)],
    # five entries, every row0, every slot; for the copy out of the pool, block 2 is read into two slots
    5: [(2, 0, 0), (0, 2, 32), (4, 1, 16), (1, 0, 32), (3, 2, 0)],
}
READ_TWICE = [(2, 0, 0), (0, 2, 32), (2, 1, 16), (1, 0, 32), (3, 2, 0)]


def _buffers(d, dt, seed):
    g = torch.Generator().manual_seed(seed)
    kv = torch.randn(LAYERS, 2, SLOTS, HEADS, CTX, d, generator=g).to(dt).to(DEV)
    pool = torch.randn(BLOCKS, LAYERS, 2, HEADS, R, d, generator=g).to(dt).to(DEV)
    return kv, pool


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_kv_blocks_copy_equals_torch_indexing_bitwise(d, dt):
    L = _lib()
    for n, table in TABLES.items():
        # slots -> pool
        kv, pool = _buffers(d, dt, 10 * n + d)
        kv0, want = kv.clone(), pool.clone()
        for b, s, r0 in table:
            want[b] = kv0[:, :, s, :, r0:r0 + R]
        L.kv_blocks_copy(kv, pool, table, to_pool=True)
        torch.cuda.synchronize()
        assert torch.equal(pool.view(torch.uint8), want.view(torch.uint8)), (n, "to_pool")      # the named blocks, and every other block unchanged
        assert torch.equal(kv.view(torch.uint8), kv0.view(torch.uint8))
        # pool -> slots (the five-entry table reads block 2 twice)
        table = READ_TWICE if n == 5 else table
        kv, pool = _buffers(d, dt, 10 * n + d + 1)
        pool0, want = pool.clone(), kv.clone()
        for b, s, r0 in table:
            want[:, :, s, :, r0:r0 + R] = pool0[b]
        L.kv_blocks_copy(kv, pool, table, to_pool=False)
        torch.cuda.synchronize()
        assert torch.equal(kv.view(torch.uint8), want.view(torch.uint8)), (n, "from_pool")      # neighbouring rows, other slots: unchanged
        assert torch.equal(pool.view(torch.uint8), pool0.view(torch.uint8))
        if n == 5:
            assert torch.equal(kv[:, :, 0, :, 0:R], kv[:, :, 1, :, R:2 * R]) and not torch.equal(kv[:, :, 0, :, R:2 * R], kv[:, :, 1, :, R:2 * R])


def test_kv_blocks_copy_wrapper_refuses_bad_tables_before_writing():
    L = _lib()
    kv, pool = _buffers(64, torch.bfloat16, 3)
    kv0, pool0 = kv.clone(), pool.clone()
    good = (1, 1, 16)
    for bad, to_pool, what in (((BLOCKS, 0, 0), True, "block"), ((-1, 0, 0), False, "block"), ((0, SLOTS, 0), True, "slot"), ((0, 0, 8), True, "row0"),
                               ((0, 0, CTX - 8), False, "row0"), ((0, 0, CTX), False, "row0"), ((0, 0, -16), True, "row0"),
                               ((1, 2, 0), True, "written twice"), ((4, 1, 16), False, "written twice")):
        with pytest.raises(ValueError, match=what):
            L.kv_blocks_copy(kv, pool, [good, bad], to_pool=to_pool)
    torch.cuda.synchronize()
    assert torch.equal(kv, kv0) and torch.equal(pool, pool0)
    L.kv_blocks_copy(kv, pool, [good, (1, 2, 0)], to_pool=False)                                 # one block into two slots is no conflict
    torch.cuda.synchronize()
    assert torch.equal(kv[:, :, 1, :, 16:32], pool0[1]) and torch.equal(kv[:, :, 2, :, 0:16], pool0[1])


# ------------------------------------------------------------------ 2. fp32: several calls on one cache against the oracle and the rules
@pytest.fixture(scope="module")
def tiny():
    from tests.test_gpu_inflight import _oracle
    from tests.test_gpu_prefix import _queue
    cfg = O.cfg_tiny()
    W = O.make_weights(cfg, seed=0)
    reqs = _queue(cfg)
    want, margin = _oracle(cfg, W, reqs)
    return cfg, W, reqs, want, margin


def _match(cfg, a, ka, c, kc):
    """the common prefix of prompt a with an earlier prompt c; at or behind c's first placeholder only under the same image (prefix._match)"""
    m = 0
    while m < min(len(a), len(c)) and a[m] == c[m]:
        m += 1
    if cfg.img_token_id in c and ka != kc:
        m = min(m, c.index(cfg.img_token_id))
    return m


def _cached_rows(cfg, prompts, keys, seen, seen_keys):
    """the lookup rule on lists: C_i = the longest chain of full 16-row blocks some earlier prompt left, in front of the last row"""
    return [max((R * (min(_match(cfg, p, keys[i], c, kc), len(p) - 1) // R) for c, kc in zip(seen, seen_keys)), default=0) for i, p in enumerate(prompts)]


def _vision(cfg, prompts, keys, P):
    tok = cfg.img_token_id
    return [keys[i] is not None and not (tok in p and max(k for k, t in enumerate(p) if t == tok) < P[i]) for i, p in enumerate(prompts)]


THIRD_BASE = 78     # seeds of the third queue's new ids, chosen on the CPU oracle: its smallest top-2 margin is 5.0e-3 (asserted >= 1e-4 below)


def _third_queue(cfg, reqs):
    """new questions about the same three images: each continues one of the first queue's questions (two per image) with 16..21 ids of its own.
    (With Q = 8 the image slot ends at row 30, inside the block [16, 32): a question that shares only head + slot with an earlier one finds ONE
    block and still needs its image; one more common row completes the second block.)"""
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    g = torch.Generator().manual_seed(THIRD_BASE)
    return [(torch.cat([reqs[k][0][0], torch.randint(3, hi, (16 + k,), generator=g)])[None], reqs[k][1], 4 + k) for k in range(6)]


def test_two_calls_and_a_third_queue_on_one_cache_fp32(tiny):
    from tests.test_gpu_inflight import _as_dicts, _oracle
    from tests.test_gpu_prefix import BASE, IMAGE_OF, _expected_rows
    cfg, W, reqs, want, margin = tiny
    assert margin >= 1e-4, f"prompt seeds {BASE}: margin {margin:.2e} -- equality of ids is not decidable here"
    prompts = [r[0][0].tolist() for r in reqs]
    T = [len(p) for p in prompts]
    Pplan, vplan, _ = _expected_rows(cfg, reqs, IMAGE_OF)
    m = make_hip_model(cfg, W, torch.float32)
    cache = m.new_prefix_cache()
    t = cfg.text
    assert cache.block_rows == 16 and cache.stats["calls"] == 0
    assert cache.nbytes == 8192 * t.num_hidden_layers * 2 * t.hidden_size * 4 and tuple(cache.pool.shape[:3]) == (512, t.num_hidden_layers, 2)
    # call 1: a cold cache -- the plan alone, and every full block of every prompt is left behind
    got = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    st1 = dict(m.last_inflight_stats)
    for i in range(14):
        assert torch.equal(got[i].cpu(), want[i]), (1, i, got[i].tolist(), want[i].tolist())
    assert st1["cache_rows_reused"] == 0 and st1["rows_reused"] == sum(Pplan) and st1["vision_runs"] == sum(vplan)
    assert st1["cache_evictions"] == 0 and st1["cache_insert_skipped"] == 0 and st1["rows_reused"] + st1["rows_computed"] == sum(T)
    distinct = {(tuple(p[:R * (k + 1)]), IMAGE_OF[i] if cfg.img_token_id in p[:R * (k + 1)] else None) for i, p in enumerate(prompts) for k in range(len(p) // R)}
    assert st1["cache_blocks_inserted"] == cache.used_blocks == len(distinct) < sum(len(p) // R for p in prompts)    # common blocks are inserted once
    # call 2: C_i rows from the cache, P_i = max(C_i, Pplan_i), vision recomputed from P_i
    C = _cached_rows(cfg, prompts, IMAGE_OF, prompts, IMAGE_OF)
    assert C == [R * ((x - 1) // R) for x in T]
    P2 = [max(c, p) for c, p in zip(C, Pplan)]
    got = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    st2 = dict(m.last_inflight_stats)
    print(f"[prefix cache] call 2: C {C} Pplan {Pplan} -> rows reused {st2['rows_reused']} (cache {st2['cache_rows_reused']}) of {sum(T)}, vision runs {st2['vision_runs']}")
    for i in range(14):
        assert torch.equal(got[i].cpu(), want[i]), (2, i, got[i].tolist(), want[i].tolist())
    assert st2["cache_rows_reused"] == sum(c for c, p in zip(C, Pplan) if c > 0 and c >= p) > 0
    assert st2["rows_reused"] == sum(P2) > st1["rows_reused"] and st2["rows_computed"] == sum(T) - sum(P2)
    assert st2["vision_runs"] == sum(_vision(cfg, prompts, IMAGE_OF, P2)) < st1["vision_runs"]
    assert st2["cache_blocks_inserted"] == 0 and st2["decode_from"] == T and st2["steps"] == st1["steps"]
    # a third queue: new questions about the same images -- no vision run at all
    third = _third_queue(cfg, reqs)
    want3, margin3 = _oracle(cfg, W, third)
    assert margin3 >= 1e-4, f"third queue, seeds {THIRD_BASE}: margin {margin3:.2e} -- pick other seeds"
    p3 = [r[0][0].tolist() for r in third]
    k3 = IMAGE_OF[:6]
    assert all(len(p3[k]) - T[k] >= 16 for k in range(6))
    C3 = _cached_rows(cfg, p3, k3, prompts, IMAGE_OF)
    Pplan3, _, _ = _expected_rows(cfg, third, k3)
    P3 = [max(c, p) for c, p in zip(C3, Pplan3)]
    got = m.generate_many(_as_dicts(third), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    st3 = dict(m.last_inflight_stats)
    for i in range(6):
        assert torch.equal(got[i].cpu(), want3[i]), (3, i, got[i].tolist(), want3[i].tolist())
    assert C3 == [32] * 6 and st3["vision_runs"] == 0 == sum(_vision(cfg, p3, k3, P3))
    assert st3["cache_rows_reused"] == sum(c for c, p in zip(C3, Pplan3) if c >= p) > 0 and st3["rows_reused"] == sum(P3)
    assert st3["cache_blocks_inserted"] == sum(len(p) // R - 2 for p in p3)
    s = cache.stats
    assert s["calls"] == 3 and s["cache_rows_reused"] == st2["cache_rows_reused"] + st3["cache_rows_reused"] and s["invalidated"] == 0
    assert s["cache_blocks_inserted"] == st1["cache_blocks_inserted"] + st3["cache_blocks_inserted"] == cache.used_blocks
    # without the cache nothing changed: today's stats, today's ids
    plain = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(plain, want)) and "cache_rows_reused" not in m.last_inflight_stats
    assert m.last_inflight_stats["rows_reused"] == sum(Pplan)
    cache.clear()
    assert cache.used_blocks == 0 and cache.stats["images"] == 0


def test_a_cache_of_four_blocks_evicts_and_keeps_the_ids_fp32(tiny):
    from tests.test_gpu_inflight import _as_dicts
    cfg, W, reqs, want, margin = tiny
    m = make_hip_model(cfg, W, torch.float32)
    cache = m.new_prefix_cache(max_tokens=64)
    assert cache.n_blocks == 4
    evictions = 0
    for call in range(3):
        got = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
        st = m.last_inflight_stats
        for i in range(14):
            assert torch.equal(got[i].cpu(), want[i]), (call, i)
        assert st["rows_reused"] + st["rows_computed"] == sum(int(r[0].shape[1]) for r in reqs)
        evictions += st["cache_evictions"]
        assert cache.used_blocks <= 4 and cache.peak_used_blocks <= 4
    assert evictions > 0 and cache.stats["cache_evictions"] == evictions and cache.stats["cache_insert_skipped"] > 0
    assert cache.stats["images"] <= 4                                # the pixel tensors leave with the last block that names them


def test_one_request_queue_on_a_warm_cache_takes_the_slots_route_fp32(tiny):
    from tests.test_gpu_inflight import _as_dicts
    cfg, W, reqs, want, margin = tiny
    m = make_hip_model(cfg, W, torch.float32)
    for i in (7, 11):                                                   # with an image, text only
        cache = m.new_prefix_cache(max_tokens=1024)
        ids, px, n = reqs[i]
        alone = m.generate(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, do_sample=False, eos_token_id=None)[0].cpu()
        assert torch.equal(alone, want[i])
        T = ids.shape[1]
        for call, reused in ((1, 0), (2, R * ((T - 1) // R))):
            got = m.generate_many(_as_dicts([reqs[i]]), do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
            st = m.last_inflight_stats
            assert torch.equal(got[0].cpu(), alone), (i, call, got[0].tolist(), alone.tolist())
            assert st["slots"] == 1 and st["cache_rows_reused"] == st["rows_reused"] == reused and st["rows_computed"] == T - reused
            assert st["vision_runs"] == (px is not None and call == 1)
    # max_batch = 1 over several requests: one slot, the cache between the calls (never inside one: lookups precede the first admission)
    cache = m.new_prefix_cache(max_tokens=1024)
    got = m.generate_many(_as_dicts(reqs[:4]), max_batch=1, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want[:4])) and m.last_inflight_stats["slots"] == 1 and m.last_inflight_stats["cache_rows_reused"] == 0
    again = m.generate_many(_as_dicts(reqs[:4]), max_batch=1, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(again, want[:4]))
    assert m.last_inflight_stats["cache_rows_reused"] == sum(R * ((int(r[0].shape[1]) - 1) // R) for r in reqs[:4]) and m.last_inflight_stats["vision_runs"] == 0
    # without a cache the one-slot route is generate() per request, sharing nothing (as before)
    m.generate_many(_as_dicts(reqs[:2]), max_batch=1, do_sample=False, eos_token_id=None, share_prefix=True)
    assert m.last_inflight_stats["rows_reused"] == 0 and "cache_rows_reused" not in m.last_inflight_stats


def test_warm_cache_graph_eager_and_per_request_configs_fp32(tiny):
    from tests.test_gpu_inflight import _as_dicts, _cut
    cfg, W, reqs, want, margin = tiny
    m = make_hip_model(cfg, W, torch.float32)
    cache = m.new_prefix_cache(max_tokens=2048)
    m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    eos = sorted({int(want[r][len(want[r]) // 2]) for r in (2, 7, 11)})
    for e in (None, eos):
        exp = [_cut(x, e) for x in want]
        for sps, graph in ((1, True), (3, True), (8, False), (3, False)):
            got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=e, use_graph=graph, share_prefix=True,
                                  prefix_cache=cache)
            assert m.last_inflight_stats["cache_rows_reused"] > 0
            for i in range(14):
                assert torch.equal(got[i].cpu(), exp[i]), (e, sps, graph, i, got[i].tolist(), exp[i].tolist())
    # two configs in one queue, seeded: request i under its own config, as without the cache
    greedy = dict(do_sample=False, eos_token_id=None, repetition_penalty=1.2)
    sampled = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, eos_token_id=None)
    mixed = [dict(d, generation_config=(greedy if i % 2 else sampled), seed=500 + i) for i, d in enumerate(_as_dicts(reqs))]
    base = m.generate_many(mixed, max_batch=4, steps_per_sync=4, do_sample=False, eos_token_id=None, share_prefix=True)
    assert m.last_inflight_stats["config_classes"] == 2
    got = m.generate_many(mixed, max_batch=4, steps_per_sync=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_cache=cache)
    assert m.last_inflight_stats["config_classes"] == 2 and m.last_inflight_stats["seeded"] == 14 and m.last_inflight_stats["cache_rows_reused"] > 0
    for i in range(14):
        assert torch.equal(got[i], base[i]), (i, got[i].tolist(), base[i].tolist())
    assert sum(not torch.equal(a.cpu(), b) for a, b in zip(got, want)) >= 4                      # the configs are no plain greedy decoding


def test_context_rebuild_invalidates_the_cache(tiny):
    from tests.test_gpu_inflight import _as_dicts
    cfg, W, reqs, want, margin = tiny
    m = make_hip_model(cfg, W, torch.float32)
    cache = m.new_prefix_cache(max_tokens=1024)
    nbytes = cache.nbytes
    kw = dict(max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True)
    m.generate_many(_as_dicts(reqs), prefix_cache=cache, **kw)
    assert cache.used_blocks > 0 and cache.stats["invalidated"] == 0
    m.half()                                                            # a dtype switch rebuilds the context: the rows describe another model
    got = m.generate_many(_as_dicts(reqs), prefix_cache=cache, **kw)
    st = dict(m.last_inflight_stats)
    ref = m.generate_many(_as_dicts(reqs), **kw)                        # nothing reused: launch for launch the uncached path in this dtype
    assert cache.stats["invalidated"] == 1 and st["cache_rows_reused"] == 0 and st["rows_reused"] == m.last_inflight_stats["rows_reused"]
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert cache.pool.dtype == torch.bfloat16 and cache.nbytes == nbytes // 2 and st["cache_blocks_inserted"] == cache.used_blocks > 0
    m.generate_many(_as_dicts(reqs), prefix_cache=cache, **kw)
    assert m.last_inflight_stats["cache_rows_reused"] > 0 and cache.stats["invalidated"] == 1
    m.float()
    got = m.generate_many(_as_dicts(reqs), prefix_cache=cache, **kw)
    assert cache.stats["invalidated"] == 2 and m.last_inflight_stats["cache_rows_reused"] == 0 and cache.pool.dtype == torch.float32


def test_prefix_cache_refusals(tiny):
    from tests.test_gpu_inflight import _as_dicts
    cfg, W, reqs, want, margin = tiny
    m = make_hip_model(cfg, W, torch.float32)
    other = make_hip_model(cfg, W, torch.float32)
    cache = m.new_prefix_cache(max_tokens=256)
    m._inflight_logits_tap = []                                         # anything admitted would leave its logits here
    with pytest.raises(ValueError, match=r"prefix_cache.*share_prefix=True"):
        m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, prefix_cache=cache)
    with pytest.raises(ValueError, match=r"prefix_cache.*another model"):
        other.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, share_prefix=True, prefix_cache=cache)
    with pytest.raises(ValueError, match=r"prefix_cache.*another model"):
        m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, share_prefix=True, prefix_cache=object())
    masked = _as_dicts(reqs)
    masked[5]["attention_mask"] = torch.ones_like(masked[5]["input_ids"])
    masked[5]["attention_mask"][0] = 0
    with pytest.raises(ValueError, match=r"share_prefix=True with an attention_mask.*request 5\)"):
        m.generate_many(masked, max_batch=4, do_sample=False, share_prefix=True, prefix_cache=cache)
    m.image_at_head = True
    with pytest.raises(ValueError, match=r"num_beams=2.*image_at_head=True"):
        m.generate_many(_as_dicts(reqs), max_batch=4, num_beams=2, share_prefix=True, prefix_cache=cache)
    m.image_at_head = False
    with pytest.raises(ValueError, match="max_tokens"):
        m.new_prefix_cache(max_tokens=8)
    assert m._inflight_logits_tap == [] and cache.used_blocks == 0 and cache.stats["calls"] == 0
    m._inflight_logits_tap = None
    ecfg = cfg_engine_small()
    m16 = make_hip_model(ecfg, O.make_weights(ecfg, seed=3), torch.bfloat16)
    c16 = m16.new_prefix_cache(max_tokens=64)
    m16.enable_fp8_decode(True, prefill=False, kv_cache=True)
    with pytest.raises(ValueError, match="e4m3"):
        m16.generate_many([dict(input_ids=torch.arange(3, 40)), dict(input_ids=torch.arange(3, 50))], max_batch=4, do_sample=False, share_prefix=True,
                          prefix_cache=c16)


# ------------------------------------------------------------------ 3. chat_many forwards the cache
from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_many_with_a_prefix_cache_equals_chat_many(loaded, capsys):  # noqa: F811
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    gc = GenerationConfig(max_new_tokens=7, do_sample=False, eos_token_id=None)
    img = _image()
    texts = ["what is this?", "hello world", "a cat sitting on a mat", "describe the image", "tiny corpus"]
    want = visualcla.chat_many(model, [(img, text) for text in texts], generation_config=gc, max_batch=3, share_prefix=True)
    cache = model.new_prefix_cache(max_tokens=1024)
    reused = []
    for call in range(2):
        got = visualcla.chat_many(model, [(img, text) for text in texts], generation_config=gc, max_batch=3, share_prefix=True, prefix_cache=cache)
        reused.append(model.last_inflight_stats["cache_rows_reused"])
        for (r1, h1), (r2, h2) in zip(want, got):
            assert r1 == r2 and h1 == h2, (call, r1, r2)
    capsys.readouterr()
    assert reused[0] == 0 and reused[1] > 0 and model.last_inflight_stats["vision_runs"] <= 1 and cache.stats["calls"] == 2
    with pytest.raises(ValueError, match=r"prefix_cache.*share_prefix=True"):
        visualcla.chat_many(model, [(img, texts[0])], generation_config=gc, prefix_cache=cache)


# ------------------------------------------------------------------ 4. bf16 at the engine widths: rows a PREVIOUS call left in the cache
def test_prefix_cache_bf16_engine_widths():
    """the form and the bounds of test_share_prefix_bf16_engine_widths, applied to requests admitted on rows a previous call left in the cache (48 of
    their 64 rows: three blocks) against the fp32 oracle on the full prompt: max < 0.12, mean < 0.022, the oracle's argmax wherever its top-2 margin
    is >= 0.24, and no further from the oracle than the same request through generate_many() without sharing (mean <= 1.25 mean0 + 1e-3)"""
    from tests.test_gpu_prefix import _shared_rows_vs_oracle
    cfg = cfg_engine_small()
    W = O.make_weights(cfg, seed=1)
    m = make_hip_model(cfg, W, torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    head = torch.randint(3, cfg.text.vocab_size - 8, (1, 40), generator=g)
    prompts = [torch.cat([head, torch.randint(3, cfg.text.vocab_size - 8, (1, 24), generator=g)], dim=1) for _ in range(4)]
    without, _ = _shared_rows_vs_oracle(m, cfg, W, prompts, False)
    cache = m.new_prefix_cache(max_tokens=512)
    plain = m.generate_many
    m.generate_many = lambda reqs, **kw: plain(reqs, prefix_cache=cache, **kw)        # the helper's own call, with the cache
    try:
        _, st1 = _shared_rows_vs_oracle(m, cfg, W, prompts, True)
        assert st1["cache_rows_reused"] == 0 and st1["cache_blocks_inserted"] == 2 + 4 * 2 and st1["rows_reused"] == 3 * 40
        with_c, st = _shared_rows_vs_oracle(m, cfg, W, prompts, True)
    finally:
        del m.generate_many
    assert st["cache_rows_reused"] == st["rows_reused"] == 4 * 48 and st["rows_computed"] == 4 * 16 and st["cache_blocks_inserted"] == 0, st
    for i in range(4):
        for s, ((mx, mean, a_hip, a_ref, margin), (mx0, mean0, *_)) in enumerate(zip(with_c[i], without[i])):
            print(f"[prefix cache bf16] request {i} step {s}: cached max {mx:.3e} mean {mean:.3e}; unshared max {mx0:.3e} mean {mean0:.3e}; oracle margin {margin:.3e}")
    for i in range(4):
        for s, ((mx, mean, a_hip, a_ref, margin), (mx0, mean0, *_)) in enumerate(zip(with_c[i], without[i])):
            assert mx < 0.12 and mean < 0.022, (i, s, mx, mean)
            assert margin < 0.24 or a_hip == a_ref, (i, s, a_hip, a_ref, margin)
            assert mean <= 1.25 * mean0 + 1e-3, (i, s, mean, mean0)

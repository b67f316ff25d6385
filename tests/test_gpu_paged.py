"""The paged K/V cache of the slots on the MI355X: vcla_attn_decode_paged bit for bit against vcla_attn_decode_rows on
a contiguous cache holding the same rows, vcla_llama_decode_slots_paged against vcla_llama_decode_slots_stops step by step, and
generate_many(kv_pool_tokens=) against the same call without a pool, against the CPU oracle and against the schedule the host simulation
predicts.  No test hands a kernel an invalid table: every table here goes through the host validation (visualcla/_lib.py kv_page_rows)."""
import ctypes as C
import random

import pytest
import torch

from oracle import visualcla_oracle as O
from tests import paged_queue as PQ
from tests.helpers import cfg_engine_small, make_hip_model
from tests.test_gpu_inflight import _oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 16


def _lib():
    from visualcla import _lib as L
    return L


def _I():
    from visualcla import inflight
    return inflight


def _scatter(rng, n_blocks, needs):
    """needs[b] blocks for every slot out of a pool of n_blocks, scattered; a slot with two or more blocks never holds them in ascending order"""
    free = list(range(n_blocks))
    rng.shuffle(free)
    out = []
    for n in needs:
        mine = [free.pop() for _ in range(n)]
        if n >= 2 and mine == sorted(mine):
            mine[0], mine[-1] = mine[-1], mine[0]
        out.append(mine)
    return out, free


def _pattern(shape, dt):
    """a tensor of `dt` whose every byte is 0x5A (a finite value in fp32 and in bf16)"""
    return torch.full((*shape[:-1], shape[-1] * torch.empty((), dtype=dt).element_size()), 0x5A, dtype=torch.uint8, device=DEV).view(dt)


def _row_index(blocks, n_rows):
    return torch.tensor([blocks[r // R] * R + r % R for r in range(n_rows)], device=DEV, dtype=torch.int64)


# ------------------------------------------------------------------ 1. the kernel, bit for bit
CTX = 640
POSITIONS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, CTX - 1, -1, CTX, 37]      # block seams, the flash kernel's batch seams, inactive rows


@pytest.mark.parametrize("dt,frag", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [3, 16, 32, 64])                   # H = 32: B * H on both sides of launch_decode's thresholds 512 and 1024
def test_attn_decode_paged_is_bitwise_attn_decode_rows(dt, frag, d, masked, B):
    L = _lib()
    lib = L.load()
    H, code, scale = 32, L.dtype_code(dt), d ** -0.5
    g = torch.Generator(device=DEV).manual_seed(B * 131 + d + masked)
    rng = random.Random(B * 7 + d + masked)
    ang = torch.rand(CTX, d // 2, generator=g, device=DEV) * 6.28
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    kv0 = (torch.randn(2, B, H, CTX, d, generator=g, device=DEV) * 0.5).to(dt)
    qkv = torch.randn(B, 3 * H * d, generator=g, device=DEV).to(dt)
    km = (torch.rand(B, CTX, generator=g, device=DEV) > 0.25).to(torch.int32) if masked else None
    pos = [POSITIONS[(b * 4 + B) % len(POSITIONS)] for b in range(B)]
    if B >= len(POSITIONS):
        assert set(pos) == set(POSITIONS)
    active = [0 <= p < CTX for p in pos]
    row_pos = torch.tensor(pos, dtype=torch.int32, device=DEV)
    # ---- the pool: every active slot owns exactly the blocks of its pos + 1 rows, scattered; spare blocks; unowned blocks hold a byte pattern
    needs = [(p + 1 + R - 1) // R if a else 0 for p, a in zip(pos, active)]
    NB = sum(needs) + 9
    blocks, spare = _scatter(rng, NB, needs)
    assert len(spare) == 9 and all(bl != sorted(bl) for bl in blocks if len(bl) >= 2)
    ld = CTX // R
    table = L.kv_page_rows(blocks, [p + 1 if a else 0 for p, a in zip(pos, active)], NB, ld).to(DEV)
    assert all(table[b, needs[b]:].eq(-1).all() for b in range(B))
    pool0 = _pattern((2, H, NB * R, d), dt)
    for b in range(B):
        if needs[b]:
            pool0[:, :, _row_index(blocks[b], needs[b] * R)] = kv0[:, b, :, :needs[b] * R]
    pages = L.kv_pages(table, NB)

    def new_out():
        if frag:
            return torch.ones((H * d) // 32, (B + 15) // 16, 64, 8, dtype=dt, device=DEV)
        return torch.ones(B, H * d, dtype=dt, device=DEV)

    def rows_of(o):
        return L.from_frag(o, B) if frag else o
    kv_r, out_r = kv0.clone(), new_out()
    L.check(lib.vcla_attn_decode_rows(qkv.data_ptr(), kv_r[0].data_ptr(), kv_r[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_r.data_ptr(), B, H, d, CTX,
                                      row_pos.data_ptr(), L.ptr(km), CTX, scale, code, frag, L.stream_ptr()))
    rows_label = L.last_launch()
    pool, out_p = pool0.clone(), new_out()
    L.check(lib.vcla_attn_decode_paged(qkv.data_ptr(), pool[0].data_ptr(), pool[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_p.data_ptr(), B, H, d, CTX,
                                       row_pos.data_ptr(), C.byref(pages), L.ptr(km), CTX, scale, code, frag, L.stream_ptr()))
    label = L.last_launch()
    # the paged instantiation of the very kernel the rows entry picked
    assert rows_label.endswith(",ROWS=true>") and label == rows_label[:-1] + ",PAGED=true>", (rows_label, label)
    assert label.startswith("attn_decode_kernel<f32," if dt == torch.float32 else "attn_decode_flash_kernel<") and f"D={d}," in label
    want, got = rows_of(out_r), rows_of(out_p)
    assert torch.equal(got, want), "output differs from vcla_attn_decode_rows on the contiguous copy"
    for b in range(B):
        if not active[b]:
            assert not got[b].any(), b                           # an inactive row: a zero output row (and no block to write into)
            continue
        mine = pool[:, :, _row_index(blocks[b], needs[b] * R)]
        assert torch.equal(mine, kv_r[:, b, :, :needs[b] * R]), f"slot {b} at {pos[b]}: its blocks differ from the contiguous cache"
        assert not torch.equal(mine[:, :, pos[b]], kv0[:, b, :, pos[b]])                      # it did append, and (above) nothing else moved
    spare_rows = torch.tensor([s * R + r for s in spare for r in range(R)], device=DEV)
    assert torch.equal(pool[:, :, spare_rows], pool0[:, :, spare_rows]), "an unowned block was written"
    assert torch.equal(table.cpu(), L.kv_page_rows(blocks, [0] * B, NB, ld))                  # the table is read only


def test_attn_decode_paged_refusals():
    L = _lib()
    lib = L.load()
    t = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    rp = torch.zeros(1, dtype=torch.int32, device=DEV)
    table = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    p = t.data_ptr()

    def call(d=64, ctx=64, pages=None, dtype=L.VCLA_BF16):
        pg = L.kv_pages(table, 4) if pages is None else pages
        L.check(lib.vcla_attn_decode_paged(p, p, p, p, p, p, 1, 1, d, ctx, rp.data_ptr(), C.byref(pg) if pg != "null" else None, None, 0, 1.0, dtype, 0, L.stream_ptr()))
    for kw, why in ((dict(dtype=L.VCLA_BF16 | 0x100), "e4m3 K/V cache is not supported"), (dict(pages="null"), "null block table"),
                    (dict(pages=L.KvPages()), "null block table"), (dict(d=32), "head dim 32 not in"), (dict(ctx=65), "does not cover ctx_cap 65")):
        with pytest.raises((ValueError, L.VclaError), match=why):
            call(**kw)
    with pytest.raises(ValueError, match="contiguous int32"):
        L.kv_pages(torch.zeros(1, 4, dtype=torch.int64, device=DEV), 4)


# ------------------------------------------------------------------ 2. the engine entry, step by step
@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("which,dt,B", [("tiny", torch.float32, 5), ("tiny", torch.bfloat16, 5), ("engine", torch.float32, 6), ("engine", torch.bfloat16, 40)])
def test_decode_slots_paged_is_bitwise_decode_slots_stops(which, dt, B, graph):
    L = _lib()
    lib = L.load()
    cfg = O.cfg_tiny() if which == "tiny" else cfg_engine_small()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=3), dt)
    t = m.config.text_config
    nL, H, d, V = t["num_hidden_layers"], t["num_attention_heads"], t["hidden_size"] // t["num_attention_heads"], t["vocab_size"]
    STEPS, ctx = 12, 128
    rng = random.Random(B)
    g = torch.Generator(device=DEV).manual_seed(B)
    T = [rng.choice([0, 1, 15, 16, 17, 31, 47, 64, 90, ctx - STEPS - 1]) for _ in range(B)]
    T[1] = -1                                                    # one slot is empty
    T[2] = 15                                                    # one crosses a block seam at its first step
    live = [p >= 0 for p in T]
    W = L.SLOT_SUMMARY_WORDS
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        kv0 = (torch.randn(nL, 2, B, H, ctx, d, generator=g, device=DEV) * 0.3).to(dt)
        km = torch.ones(B, ctx, dtype=torch.int32, device=DEV)
        km[0, :min(T[0], 3)] = 0                                 # the pad holes of a left-padded slot
        needs = [(p + STEPS + 1 + R - 1) // R if a else 0 for p, a in zip(T, live)]      # what admission reserves: T + budget rows
        NB = sum(needs) + 5
        blocks, spare = _scatter(rng, NB, needs)
        table = L.kv_page_rows(blocks, [p + STEPS + 1 if a else 0 for p, a in zip(T, live)], NB, ctx // R).to(DEV)
        pool0 = _pattern((nL, 2, H, NB * R, d), dt)
        for b in range(B):
            if needs[b]:
                pool0[:, :, :, _row_index(blocks[b], needs[b] * R)] = kv0[:, :, b, :, :needs[b] * R]
        assert lib.vcla_kv_pool_bytes(m._ctx, NB) == pool0.numel() * pool0.element_size()
        ids0 = torch.randint(3, V - 8, (B,), generator=torch.Generator().manual_seed(3)).to(DEV)
        init = torch.tensor(T + [1 if a else 0 for a in live] + [1 if a else -1 for a in live] + [STEPS + 2] * B + [0] * W, dtype=torch.int32, device=DEV)

        def drive(paged):
            """12 calls of one step each -> per step (state words, current ids, the whole workspace: logits and every activation)"""
            kv = pool0.clone() if paged else kv0.clone()
            st, cur, hist = init.clone(), ids0.clone(), torch.zeros(STEPS + 2, B, dtype=torch.int64, device=DEV)
            ws = torch.zeros(lib.vcla_llama_workspace_bytes(m._ctx, B, 1) + 512, dtype=torch.uint8, device=DEV)
            slots = L.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
            pages = L.kv_pages(table, NB)
            snaps = []
            for _ in range(STEPS):
                args = (m._ctx, C.byref(slots), 1, kv.data_ptr(), ctx, km.data_ptr(), ws.data_ptr(), ws.numel(), graph, None, None, None, None, None, None)
                if paged:
                    L.check(lib.vcla_llama_decode_slots_paged(*args, C.byref(pages), L.stream_ptr()))
                else:
                    L.check(lib.vcla_llama_decode_slots_stops(*args, L.stream_ptr()))
                snaps.append((st.tolist(), cur.tolist(), ws.clone()))
            return snaps, hist, kv
        ref, hist_r, kv_r = drive(False)
        got, hist_p, kv_p = drive(True)
        for step, (a, b) in enumerate(zip(ref, got)):
            assert a[0] == b[0] and a[1] == b[1], step           # positions, counts and the ids taken
            assert torch.equal(a[2], b[2]), f"step {step}: the workspace (logits and activations) differs"
        assert torch.equal(hist_r, hist_p) and ref[-1][0][:B] == [p + STEPS if a else -1 for p, a in zip(T, live)]
        for b in range(B):
            if needs[b]:
                assert torch.equal(kv_p[:, :, :, _row_index(blocks[b], needs[b] * R)], kv_r[:, :, b, :, :needs[b] * R]), b
        spare_rows = torch.tensor([s * R + r for s in spare for r in range(R)], device=DEV)
        assert torch.equal(kv_p[:, :, :, spare_rows], pool0[:, :, :, spare_rows])
        # pages NULL is the stops entry
        st, cur, hist = init.clone(), ids0.clone(), torch.zeros(STEPS + 2, B, dtype=torch.int64, device=DEV)
        ws = torch.zeros_like(ref[0][2])
        kv = kv0.clone()
        slots = L.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
        L.check(lib.vcla_llama_decode_slots_paged(m._ctx, C.byref(slots), STEPS, kv.data_ptr(), ctx, km.data_ptr(), ws.data_ptr(), ws.numel(), graph, None, None, None,
                                                  None, None, None, None, L.stream_ptr()))
        assert torch.equal(hist, hist_r) and torch.equal(kv, kv_r)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. end to end, fp32
BASE = 300
_REF = {}


def _requests(cfg):
    Q = cfg.resampler.num_query_tokens
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    reqs = []
    for r in range(PQ.N):
        if r % 2 == 0:
            px, ids, _ = O.make_inputs(cfg, 1, 32 + 3 * r + Q, seed_ids=BASE + r)
        else:
            px, ids = None, torch.randint(3, hi, (1, 20 + 3 * r), generator=torch.Generator().manual_seed(BASE + r))
        reqs.append((ids, px, PQ.BUDGETS[r]))
    assert [int(ids.numel()) for ids, _, _ in reqs] == PQ.prompt_lens(Q)
    return reqs


def _dicts(reqs, **extra):
    return [dict(input_ids=ids[0], pixel_values=None if px is None else px[0], max_new_tokens=n, **extra) for ids, px, n in reqs]


def _ref(dt=torch.float32):
    """(cfg, requests, the model, the run of the queue without a pool, its stats) -- once per dtype; fp32: the oracle's ids and margin first"""
    if dt not in _REF:
        cfg = O.cfg_tiny()
        W = O.make_weights(cfg, seed=0)
        reqs = _requests(cfg)
        if dt == torch.float32:
            want, margin = _oracle(cfg, W, reqs)
            print(f"[paged] smallest top-2 margin over {sum(PQ.BUDGETS)} steps = {margin:.3e}")
            assert margin >= 1e-4, f"prompt seeds {BASE}: margin {margin:.2e} -- pick other seeds, equality of ids is not decidable here"
        m = make_hip_model(cfg, W, dt)
        base = [x.tolist() for x in m.generate_many(_dicts(reqs), max_batch=PQ.MAX_BATCH, steps_per_sync=3, do_sample=False, eos_token_id=None)]
        st = dict(m.last_inflight_stats)
        assert "kv_pool_blocks" not in st and "kv_bytes" not in st
        if dt == torch.float32:
            assert base == [w.tolist() for w in want]
        _REF[dt] = (cfg, reqs, m, base, st)
    return _REF[dt]


@pytest.mark.parametrize("graph", [True, False])
def test_generate_many_with_a_pool_equals_the_call_without_fp32(graph):
    I = _I()
    cfg, reqs, m, base, _ = _ref()
    Q = cfg.resampler.num_query_tokens
    T, img = PQ.prompt_lens(Q), PQ.has_image()
    for sps in (1, 3, 8):
        kw = dict(max_batch=PQ.MAX_BATCH, steps_per_sync=sps, do_sample=False, eos_token_id=None, use_graph=graph)
        free = m.generate_many(_dicts(reqs), **kw)
        st0 = dict(m.last_inflight_stats)
        assert [x.tolist() for x in free] == base
        # ---- an ample pool: the same results, the same admission groups, nothing waits
        got = m.generate_many(_dicts(reqs), kv_pool_tokens=PQ.ample_pool_tokens(Q, st0["ctx_max"]), **kw)
        st = dict(m.last_inflight_stats)
        assert [x.tolist() for x in got] == base, (graph, sps)
        assert st["admission_waits_blocks"] == 0 and st["kv_blocks_peak"] <= st["kv_pool_blocks"] == PQ.MAX_BATCH * st0["ctx_max"] // 16
        for k in ("admission_groups", "steps", "tokens", "slot_steps_active", "slot_steps_total", "decode_from", "ctx_max", "slots"):
            assert st[k] == st0[k], (k, st[k], st0[k])
        row_bytes = 2 * cfg.text.num_hidden_layers * cfg.text.hidden_size * 4
        assert st["kv_bytes"] == st["kv_pool_blocks"] * 16 * row_bytes == st["kv_bytes_contiguous"] == PQ.MAX_BATCH * st0["ctx_max"] * row_bytes
        # ---- the tight pool: the head of the queue waits, the results are still equal, the schedule is the one the host simulation predicts
        tight = PQ.tight_pool_tokens(Q)
        got = m.generate_many(_dicts(reqs), kv_pool_tokens=tight, **kw)
        st = dict(m.last_inflight_stats)
        assert [x.tolist() for x in got] == base, (graph, sps)
        assert st["admission_waits_blocks"] > 0 and st["kv_blocks_peak"] <= st["kv_pool_blocks"] == tight // 16
        assert st["kv_bytes"] == tight * row_bytes < st["kv_bytes_contiguous"]
        sim, _ = I.simulate(PQ.BUDGETS, PQ.MAX_BATCH, sps, prompt_lens=T, has_image=img, max_position_embeddings=cfg.text.max_position_embeddings, kv_pool_tokens=tight)
        for k in ("admission_waits_blocks", "kv_blocks_peak", "kv_rows_reserved_peak", "steps", "admission_groups"):
            assert st[k] == sim.stats[k], (k, st[k], sim.stats[k])
    # the allocator of the last run ended empty (the scheduler is gone with the call: its stats are what is left) -- and the model still serves the plain call
    assert [x.tolist() for x in m.generate_many(_dicts(reqs), max_batch=PQ.MAX_BATCH, do_sample=False, eos_token_id=None)] == base


def test_the_allocator_is_empty_when_the_call_returns(monkeypatch):
    from visualcla import slots_run
    cfg, reqs, m, base, _ = _ref()
    seen = []
    run0 = slots_run.SlotsRun.run

    def run(self):
        out = run0(self)
        seen.append((self.sched.pool.used, self.sched.pool.available, len(self.sched.blocks), self.sched.pool.n_blocks))
        return out
    monkeypatch.setattr(slots_run.SlotsRun, "run", run)
    tight = PQ.tight_pool_tokens(cfg.resampler.num_query_tokens)
    calls = []
    got = m.generate_many(_dicts(reqs), max_batch=PQ.MAX_BATCH, steps_per_sync=3, do_sample=False, eos_token_id=None, kv_pool_tokens=tight,
                          on_tokens=lambda i, t, f: calls.append(i) or i in (5, 10))
    assert seen == [(0, tight // 16, 0, tight // 16)] and m.last_inflight_stats["cancelled"] == 2
    assert all(g.tolist() == b[:len(g)] for g, b in zip(got, base))


def test_one_request_with_a_pool_takes_the_slots_route():
    cfg, reqs, m, base, _ = _ref()
    one = m.generate_many(_dicts(reqs[6:7]), do_sample=False, eos_token_id=None, kv_pool_tokens=128)
    st = m.last_inflight_stats
    need = _I().blocks_for(PQ.prompt_lens(cfg.resampler.num_query_tokens)[6] + PQ.BUDGETS[6])
    assert one[0].tolist() == base[6] and st["slots"] == 1 and "admission_s" in st and st["kv_pool_blocks"] == 8 and st["kv_blocks_peak"] == need == 6
    two = m.generate_many(_dicts(reqs[6:8]), max_batch=1, do_sample=False, eos_token_id=None, kv_pool_tokens=128)
    assert [x.tolist() for x in two] == base[6:8] and m.last_inflight_stats["slots"] == 1 and "kv_bytes" in m.last_inflight_stats


# ------------------------------------------------------------------ 4. beside the other features (fp32 and bf16, bit for bit: the schedule is the same and the kernel is bitwise)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_a_pool_beside_logprobs_choices_stops_sampling_and_cancel(dt):
    cfg, reqs, m, base, st0 = _ref(dt)
    ample = PQ.ample_pool_tokens(cfg.resampler.num_query_tokens, st0["ctx_max"])
    kw = dict(max_batch=PQ.MAX_BATCH, steps_per_sync=3, do_sample=False, eos_token_id=2)
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    tok = lambda k: 3 + (k * 37) % (hi - 3)                      # noqa: E731

    def both(make, **extra):
        out = []
        for pool in (None, ample):
            out.append(m.generate_many(make(), **dict(kw, **extra), **({} if pool is None else dict(kv_pool_tokens=pool))))
            assert ("kv_pool_blocks" in m.last_inflight_stats) == (pool is not None)
        assert m.last_inflight_stats["admission_waits_blocks"] == 0
        return out
    # logprobs=5: every array bit for bit
    a, b = both(lambda: _dicts(reqs), logprobs=5)
    for i, (x, y) in enumerate(zip(a, b)):
        assert all(torch.equal(p, q) for p, q in zip(x, y)), i
    # choices on two requests, stop sequences drawn from the free run on three
    def constrained():
        q = _dicts(reqs)
        q[3]["choices"] = [[tok(1), tok(2), tok(3), tok(4)], [tok(1), tok(5)]]
        q[8]["choices"] = [[tok(7), tok(8)]]
        for i in (4, 6, 10):
            q[i]["stop_sequences"] = [base[i][3:5]]
        return q
    a, b = both(constrained)
    assert [x.tolist() for x in a] == [x.tolist() for x in b] and a[8].tolist()[:2] == [tok(7), tok(8)]
    assert len(b[4]) <= 5 and m.last_inflight_stats["stop_hits"] >= 3 and m.last_inflight_stats["constrained_requests"] == 2
    # seeded sampling under per-request configs
    def sampled():
        q = _dicts(reqs)
        for i, r in enumerate(q):
            r["seed"] = 100 + i
            if i % 3 == 1:
                r["generation_config"] = dict(do_sample=True, top_k=5, temperature=0.7)
            elif i % 3 == 2:
                r["generation_config"] = dict(do_sample=False, repetition_penalty=1.2)
        return q
    a, b = both(sampled, do_sample=True, top_k=40, top_p=0.95, temperature=0.9)
    assert [x.tolist() for x in a] == [x.tolist() for x in b] and m.last_inflight_stats["config_classes"] == 3
    # on_tokens cancelling two requests
    a, b = both(lambda: _dicts(reqs), on_tokens=lambda i, t, f: i in (6, 11))
    assert [x.tolist() for x in a] == [x.tolist() for x in b] and m.last_inflight_stats["cancelled"] == 2 and len(b[6]) < PQ.BUDGETS[6]


# ------------------------------------------------------------------ 5. refusals on the device model: nothing is launched
def test_refusals_launch_nothing():
    cfg, reqs, m, base, _ = _ref()
    m._inflight_logits_tap = []
    try:
        kw = dict(max_batch=PQ.MAX_BATCH, do_sample=False, eos_token_id=None)
        with pytest.raises(ValueError, match="kv_pool_tokens with share_prefix=True"):
            m.generate_many(_dicts(reqs), kv_pool_tokens=4096, share_prefix=True, **kw)
        with pytest.raises(ValueError, match="kv_pool_tokens with prefix_cache"):
            m.generate_many(_dicts(reqs), kv_pool_tokens=4096, share_prefix=True, prefix_cache=m.new_prefix_cache(256), **kw)
        small = PQ.tight_pool_tokens(cfg.resampler.num_query_tokens) - 16
        with pytest.raises(ValueError, match=r"kv_pool_tokens=80: a pool of 5 blocks of 16 rows cannot hold request 6 \(58 \+ 24 rows = 6 blocks\), 8 \(64 \+ 17 rows = 6 blocks\), "
                                             r"10 \(70 \+ 24 rows = 6 blocks\), 12 \(76 \+ 6 rows = 6 blocks\)$"):
            m.generate_many(_dicts(reqs), kv_pool_tokens=small, **kw)
        for bad in (0, -1, True, 64.0):
            with pytest.raises(ValueError, match="kv_pool_tokens must be None or a positive integer"):
                m.generate_many(_dicts(reqs), kv_pool_tokens=bad, **kw)
        assert m._inflight_logits_tap == []
    finally:
        m._inflight_logits_tap = None

"""In-flight batching on the GPU: the per-row decode attention against the uniform entry row by row (bit-identical), the slot bookkeeping
kernel against the host model, the per-row sampler against per-row calls of vcla_sample, and generate_many / chat_many against generate() /
chat() of every request alone and against the CPU oracle."""
import ctypes as C
import dataclasses
import random

import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from visualcla import _lib as L
    return L


# ------------------------------------------------------------------ 1. per-row positions in the decode attention
CTX = 640
POSITIONS = [0, 1, 255, 256, 257, 511, 512, 513, CTX - 1, -1, CTX, 37]      # -1 / CTX: inactive rows


@pytest.mark.parametrize("dt,frag", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [3, 15, 16, 31, 32, 64])           # H = 32: B * H on each side of launch_decode's thresholds 512 and 1024
def test_attn_decode_rows_equals_uniform_calls(dt, frag, d, masked, B):
    L = _lib()
    lib = L.load()
    H, code, scale = 32, L.dtype_code(dt), d ** -0.5
    g = torch.Generator(device=DEV).manual_seed(B * 131 + d + masked)
    ang = torch.rand(CTX, d // 2, generator=g, device=DEV) * 6.28
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    kv0 = (torch.randn(2, B, H, CTX, d, generator=g, device=DEV) * 0.5).to(dt)
    qkv = torch.randn(B, 3 * H * d, generator=g, device=DEV).to(dt)
    km = None
    if masked:
        km = (torch.rand(B, CTX, generator=g, device=DEV) > 0.25).to(torch.int32)
    pos = [POSITIONS[(b * 5 + B) % len(POSITIONS)] for b in range(B)]
    if B >= len(POSITIONS):
        assert set(pos) == set(POSITIONS)
    row_pos = torch.tensor(pos, dtype=torch.int32, device=DEV)

    def new_out():
        if frag:
            return torch.ones((H * d) // 32, (B + 15) // 16, 64, 8, dtype=dt, device=DEV)
        return torch.ones(B, H * d, dtype=dt, device=DEV)

    def rows_of(o):
        return L.from_frag(o, B) if frag else o
    kv_r, out_r = kv0.clone(), new_out()
    L.check(lib.vcla_attn_decode_rows(qkv.data_ptr(), kv_r[0].data_ptr(), kv_r[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_r.data_ptr(), B, H, d, CTX,
                                      row_pos.data_ptr(), L.ptr(km), CTX, scale, code, frag, L.stream_ptr()))
    got = rows_of(out_r)
    for p in sorted(set(pos)):
        rows = [b for b in range(B) if pos[b] == p]
        if p < 0 or p >= CTX:                                    # inactive: cache bytes unchanged, output row zero
            for b in rows:
                assert torch.equal(kv_r[:, b], kv0[:, b]) and not got[b].any(), (p, b)
            continue
        kv_u, out_u = kv0.clone(), new_out()
        L.check(lib.vcla_attn_decode_fused(qkv.data_ptr(), kv_u[0].data_ptr(), kv_u[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_u.data_ptr(), B, H, d,
                                           CTX, p, None, L.ptr(km), CTX, scale, code, frag, L.stream_ptr()))
        want = rows_of(out_u)
        for b in rows:
            assert torch.equal(got[b], want[b]), f"pos {p} row {b}: output differs from the uniform call"
            assert torch.equal(kv_r[:, b], kv_u[:, b]), f"pos {p} row {b}: cache row differs from the uniform call"
            assert not torch.equal(kv_r[:, b, :, p], kv0[:, b, :, p])                     # it did append


def test_attn_decode_rows_refuses_the_e4m3_cache():
    L = _lib()
    t = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    rp = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises((ValueError, L.VclaError)):
        L.check(L.load().vcla_attn_decode_rows(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 1, 64, 64, rp.data_ptr(), None,
                                               0, 1.0, L.VCLA_BF16 | 0x100, 0, L.stream_ptr()))


# ------------------------------------------------------------------ 2. the bookkeeping kernel against the host model
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_slot_step_kernel_vs_host(dt):
    from visualcla import inflight as I
    L = _lib()
    lib = L.load()
    rng = random.Random(23)
    V, D = 97, 64
    table = torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)
    n_eos = n_budget = n_inactive = n_cont = 0
    for case in range(150):
        B = rng.choice([1, 2, 5, 16, 33, 64, 70])
        cap = rng.randint(2, 12)
        eos = rng.choice([[], [2], [2, 3, 5]])
        row_pos = [rng.choice([-1, rng.randint(0, 500)]) for _ in range(B)]
        count = [rng.randint(1, cap - 1) for _ in range(B)]
        budget = [min(cap, c + rng.choice([1, 1, 2, 5])) for c in count]
        cur = [rng.randint(0, V - 1) for _ in range(B)]
        hist = [[rng.randint(0, V - 1) for _ in range(B)] for _ in range(cap)]
        hl = [c if p >= 0 else -1 for c, p in zip(count, row_pos)]
        st = torch.tensor(row_pos + count + hl + budget + [0] * L.SLOT_SUMMARY_WORDS, dtype=torch.int32, device=DEV)
        hist_t = torch.tensor(hist, dtype=torch.int64, device=DEV)
        cur_t = torch.tensor(cur, dtype=torch.int64, device=DEV)
        x = torch.zeros(B, D, dtype=dt, device=DEV)
        a = L.slot_args(eos, st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist_t, cur_t, st[4 * B:])
        for step in range(3):
            ids = [rng.randint(0, 6) for _ in range(B)]
            ids_t = torch.tensor(ids, dtype=torch.int64, device=DEV)
            before = list(row_pos)
            L.check(lib.vcla_slot_step(ids_t.data_ptr(), C.byref(a), table.data_ptr(), x.data_ptr(), D, V, L.dtype_code(dt), L.stream_ptr()))
            n_act = I.slot_step_model(ids, row_pos, count, budget, hist, cur, eos, hl)
            s = st.tolist()
            assert s[:B] == row_pos and s[B:2 * B] == count and s[2 * B:3 * B] == hl and s[3 * B:4 * B] == budget, (case, step)
            assert s[4 * B] == n_act and s[4 * B + 1] == 0, (case, step)
            assert hist_t.tolist() == hist and cur_t.tolist() == cur, (case, step)
            assert torch.equal(x.float(), table[cur_t].float()), (case, step)          # every row: the embedding of its current id
            for b in range(B):
                fin = before[b] >= 0 and row_pos[b] < 0
                n_eos += fin and ids[b] in eos
                n_budget += fin and count[b] >= budget[b]
                n_inactive += before[b] < 0
                n_cont += row_pos[b] >= 0
    assert n_eos > 20 and n_budget > 20 and n_inactive > 100 and n_cont > 100


# ------------------------------------------------------------------ 3. per-row history length in the sampler
def test_sample_rows_vs_sample_per_row():
    from tests.test_sampling_oracle import CFGS
    L = _lib()
    lib = L.load()
    B, V, cap = 7, 4099, 48
    g = torch.Generator().manual_seed(5)
    lens = [0, 3, -1, 47, 20, 1, -5]
    for ci, cfg in enumerate(CFGS):
        logits = (torch.randn(B, V, generator=g) * 3).to(DEV)
        hist = torch.randint(0, 9, (cap, B), generator=g).to(DEV)
        uni = torch.rand(cap, B, generator=g).to(DEV)
        kw = dict(repetition_penalty=cfg.repetition_penalty, no_repeat_ngram_size=cfg.no_repeat_ngram_size, min_new_tokens=cfg.min_new_tokens, eos_ids=cfg.eos_ids,
                  temperature=cfg.temperature, top_k=cfg.top_k, top_p=cfg.top_p, min_tokens_to_keep=cfg.min_tokens_to_keep)
        kid = torch.full((B, L.SAMPLE_KEPT_LD), -1, dtype=torch.int64, device=DEV)
        nk = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        out = torch.full((B,), -9, dtype=torch.int64, device=DEV)
        a = L.sample_args(uniforms=uni, history=hist, kept_ids=kid, n_kept=nk, **kw)
        lg = logits.clone()
        L.check(lib.vcla_sample_rows(lg.data_ptr(), V, B, V, torch.tensor(lens, dtype=torch.int32, device=DEV).data_ptr(), C.byref(a), out.data_ptr(), L.stream_ptr()))
        for b, h in enumerate(lens):
            if h < 0:
                assert int(out[b]) == -9 and int(nk[b]) == -1 and torch.equal(lg[b], logits[b]), (ci, b)        # skipped: nothing touched
                continue
            hb, ub = hist[:, b:b + 1].contiguous(), uni[:, b:b + 1].contiguous()
            kid1 = torch.full((1, L.SAMPLE_KEPT_LD), -1, dtype=torch.int64, device=DEV)
            nk1 = torch.zeros(1, dtype=torch.int32, device=DEV)
            a1 = L.sample_args(uniforms=ub, history=hb, kept_ids=kid1, n_kept=nk1, **kw)
            want = L.sample(logits[b:b + 1].clone(), a1, n_hist=h)
            n = int(nk1[0])
            assert int(out[b]) == int(want[0]) and int(nk[b]) == n and torch.equal(kid[b, :n], kid1[0, :n]), (ci, b, h)


# ------------------------------------------------------------------ 4. end to end, fp32, against generate() alone and the oracle
BUDGETS = [1, 2, 5, 9, 14, 20, 26, 31, 35, 38, 40, 40]
BASE = 300          # seeds of the prompts: the smallest top-2 margin over all generated steps is checked below, before anything is compared


def _requests(cfg, base=BASE):
    Q = cfg.resampler.num_query_tokens
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    reqs = []
    for r in range(12):
        if r % 2 == 0:
            px, ids, _ = O.make_inputs(cfg, 1, 32 + 3 * r + Q, seed_ids=base + r)
        else:
            px, ids = None, torch.randint(3, hi, (1, 20 + 3 * r), generator=torch.Generator().manual_seed(base + r))
        reqs.append((ids, px, BUDGETS[r]))
    return reqs


def _oracle(cfg, W, reqs):
    """greedy ids of every request alone on the CPU oracle, and the smallest top-2 logit margin over all their steps"""
    outs, margin = [], float("inf")
    for ids, px, n in reqs:
        toks, logits = O.visualcla_generate(ids, px, torch.ones_like(ids), W, cfg, max_new_tokens=n, return_logits=True)
        for lg in logits:
            top2 = lg[0].topk(2).values
            margin = min(margin, float(top2[0] - top2[1]))
        outs.append(toks[0])
    return outs, margin


def _cut(toks, eos):
    if eos is None:
        return toks
    hit = torch.isin(toks, torch.tensor(eos)).nonzero()
    return toks if not len(hit) else toks[:int(hit[0]) + 1]


def _as_dicts(reqs):
    return [dict(input_ids=ids[0], pixel_values=None if px is None else px[0], max_new_tokens=n) for ids, px, n in reqs]


@pytest.mark.parametrize("which", ["tiny", "small"])
def test_generate_many_equals_generate_alone_and_oracle_fp32(which):
    from visualcla.inflight import step_bound
    cfg = O.cfg_tiny() if which == "tiny" else O.cfg_small()
    W = O.make_weights(cfg, seed=0)
    reqs = _requests(cfg)
    want, margin = _oracle(cfg, W, reqs)
    print(f"[inflight] {which}: smallest top-2 margin over {sum(BUDGETS)} steps = {margin:.3e}")
    assert margin >= 1e-4, f"prompt seeds {BASE}: margin {margin:.2e} -- pick other seeds, equality of ids is not decidable here"
    m = make_hip_model(cfg, W, torch.float32)
    eos = sorted({int(want[r][len(want[r]) // 2]) for r in (7, 9, 11)})      # ids plain greedy produces: they end some requests early
    n_early = 0
    for e in (None, eos):
        exp = [_cut(t, e) for t in want]
        n_early += sum(len(a) < len(b) for a, b in zip(exp, want))
        alone = [m.generate(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, do_sample=False, eos_token_id=e)[0].cpu()
                 for ids, px, n in reqs]
        for i in range(12):
            assert torch.equal(alone[i], exp[i]), (e, i)
        for sps in (1, 3, 8):
            got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=e)
            st = m.last_inflight_stats
            for i in range(12):
                assert torch.equal(got[i].cpu(), exp[i]), (e, sps, i, got[i].tolist(), exp[i].tolist())
            assert st["requests"] == 12 and st["slots"] == 4 and st["tokens"] == sum(len(x) for x in exp)
            assert st["steps"] <= step_bound([len(x) for x in exp], 4, sps), st
            assert 0 < st["slot_steps_active"] <= st["slot_steps_total"] == 4 * st["steps"]
        eager = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=e, use_graph=False)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(eager, exp))
    assert n_early >= 3
    # max_batch = 1 and a single request take generate() itself
    one = m.generate_many(_as_dicts(reqs[:3]), max_batch=1, do_sample=False, eos_token_id=None)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(one, want[:3])) and m.last_inflight_stats["slots"] == 1
    # a request that cannot fit raises with its index before anything runs
    long_ids = torch.randint(3, 50, (cfg.text.max_position_embeddings,))
    with pytest.raises(ValueError, match="request 1"):
        m.generate_many([_as_dicts(reqs)[1], dict(input_ids=long_ids)], do_sample=False)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate_many(_as_dicts(reqs), num_beams=2)
    with pytest.raises(ValueError, match="streamer"):
        m.generate_many(_as_dicts(reqs), streamer=object())
    assert m.generate_many([], do_sample=False) == []


# ------------------------------------------------------------------ 5. the sampler path without randomness
def test_generate_many_sampler_path_equals_generate():
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    reqs = _requests(cfg)
    kw = dict(do_sample=True, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=3, min_new_tokens=4)
    plain = m.generate(input_ids=reqs[11][0].cuda(), max_new_tokens=40, eos_token_id=None, **kw)[0].cpu()
    for eos in (None, int(plain[6])):
        alone = [m.generate(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, eos_token_id=eos, **kw)[0].cpu() for ids, px, n in reqs]
        if eos is not None:
            assert all(len(a) >= min(4, n) for a, (_, _, n) in zip(alone, reqs))          # the floor of min_new_tokens holds per request
        for sps in (2, 8):
            got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, eos_token_id=eos, **kw)
            for i in range(12):
                assert torch.equal(got[i].cpu(), alone[i]), (eos, sps, i)
    # real sampling runs and respects the budgets (the random stream differs from generate()'s by construction)
    torch.manual_seed(0)
    got = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=True, top_k=40, top_p=0.9, temperature=0.7, eos_token_id=None)
    assert [len(x) for x in got] == BUDGETS


# ------------------------------------------------------------------ 6. bf16 / W8A16 at the LLaMA-7B widths, rows crossing 512 keys
@pytest.mark.parametrize("fp8", [False, True])
def test_generate_many_bf16_engine_widths(fp8):
    from tests.test_gpu_lookup import _greedy_step_gaps
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=1024))
    m = make_hip_model(cfg, O.make_weights(cfg, seed=2), torch.bfloat16)
    if fp8:
        m.enable_fp8_decode(True, prefill=False)
    g = torch.Generator().manual_seed(1)
    rng = random.Random(4)
    reqs = []
    for r in range(20):
        T = [505, 498, 490][r % 7] if r % 7 < 3 else rng.randint(20, 300)       # the long ones cross 512 keys while decoding
        reqs.append((torch.randint(3, 4000, (1, T), generator=g), None, rng.randint(18, 40)))
    got = m.generate_many(_as_dicts(reqs), max_batch=8, steps_per_sync=8, do_sample=False, eos_token_id=None)
    assert [len(x) for x in got] == [n for _, _, n in reqs] and m.last_inflight_stats["slots"] == 8
    assert any(ids.shape[1] < 512 < ids.shape[1] + n for ids, _, n in reqs)
    decode_from = m.last_inflight_stats["decode_from"]
    assert any(p > ids.shape[1] for p, (ids, _, _) in zip(decode_from, reqs))          # some rows did run left-padded
    for (ids, _, n), toks, p0 in zip(reqs, got, decode_from):
        toks = toks.cpu()[None]
        if not fp8:
            # teacher-forced on the slots' own tokens: forward() must pick the same id wherever its top-2 gap is clear.  forward() is given the
            # row as the slot ran it -- left-padded to the position it decoded from, pads masked -- because in bf16 a position shift is the same
            # function only up to the rounding of the RoPE tables: against the UNPADDED prompt one of the 527 steps (request 2, T = 490 in a
            # group of T = 505, step 3, gap 0.067) differs, and generate() on the same left-padded batch of 8 differs there in the same way.
            pad = p0 - ids.shape[1]
            full = torch.cat([torch.zeros(1, pad, dtype=torch.int64), ids, toks[:, :-1]], dim=1)
            mask = torch.cat([torch.zeros(1, pad, dtype=torch.int64), torch.ones(1, full.shape[1] - pad, dtype=torch.int64)], dim=1)
            lg = m(input_ids=full.cuda(), attention_mask=mask.cuda()).logits[0].float()
            rows = lg[p0 - 1:p0 - 1 + n]
            top2 = rows.topk(2, dim=-1).values
            clear = ((top2[:, 0] - top2[:, 1]) >= 0.05).cpu()
            assert torch.equal(rows.argmax(dim=-1).cpu()[clear], toks[0][clear])
        else:
            # forward() runs the bf16 weights: the reference is the greedy step path on the fp8 copies, up to its first near-tie
            steps, gap = _greedy_step_gaps(m, ids, n)
            first_tie = int((gap < 0.05).nonzero()[0]) if bool((gap < 0.05).any()) else n
            assert torch.equal(toks[0, :first_tie], steps[0, :first_tie])


# ------------------------------------------------------------------ 7. neighbours keep working
def test_neighbours_unchanged_by_generate_many():
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    reqs = _requests(cfg)
    px4, ids4, _ = O.make_inputs(cfg, 4, 48, seed_ids=9)
    ids1 = reqs[11][0].cuda()

    def neighbours():
        a = m.generate(input_ids=ids1, max_new_tokens=24, do_sample=False, eos_token_id=None).cpu()
        b = m.generate(input_ids=ids4.cuda(), pixel_values=px4.cuda(), max_new_tokens=16, do_sample=False, eos_token_id=None).cpu()
        c = m.generate(input_ids=ids1, max_new_tokens=24, do_sample=False, eos_token_id=None, prompt_lookup_num_tokens=3).cpu()
        return a, b, c
    before = neighbours()
    first = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None)
    after = neighbours()
    again = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None)
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert torch.equal(before[0], before[2]) and all(torch.equal(x, y) for x, y in zip(first, again))


from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_many_equals_chat(loaded, capsys):  # noqa: F811
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    gc = GenerationConfig(max_new_tokens=7, do_sample=False, eos_token_id=None)
    img = _image()
    texts = ["what is this?", "hello world", "a cat sitting on a mat", "describe the image", "tiny corpus"]
    want = []
    for k, text in enumerate(texts):
        hist = [] if k != 2 else [{"type": "instruction", "value": "hello", "first_instruction": True}, {"type": "response", "value": "a cat"}]
        want.append(visualcla.chat(model, img, text, history=hist, generation_config=gc))
    capsys.readouterr()
    items = [(img, text) if k != 2 else (img, text, [{"type": "instruction", "value": "hello", "first_instruction": True}, {"type": "response", "value": "a cat"}])
             for k, text in enumerate(texts)]
    got = visualcla.chat_many(model, items, generation_config=gc, max_batch=3)
    assert len(got) == len(want)
    for (r1, h1), (r2, h2) in zip(want, got):
        assert r1 == r2 and h1 == h2
    assert got[2][1] is items[2][2] and len(got[2][1]) == 4

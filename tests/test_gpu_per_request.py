"""Per-request generation configs and seeds on the GPU: the sampler with one parameter record per row against
vcla_sample row by row (bit-identical), the slot bookkeeping with one eos list per slot against the host model, and generate_many /
chat_many under mixed configs against generate() / chat() of every request alone under its own config and against uniform-config queues."""
import ctypes as C
import dataclasses
import random

import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model
from tests.test_gpu_inflight import BUDGETS, _as_dicts, _cut, _oracle, _requests

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from visualcla import _lib as L
    return L


def _kw(cfg):
    return dict(repetition_penalty=cfg.repetition_penalty, no_repeat_ngram_size=cfg.no_repeat_ngram_size, min_new_tokens=cfg.min_new_tokens, eos_ids=cfg.eos_ids,
                temperature=cfg.temperature, top_k=cfg.top_k, top_p=cfg.top_p, min_tokens_to_keep=cfg.min_tokens_to_keep)


# ------------------------------------------------------------------ 1. one parameter record per row in the sampler
def _table_vs_rows(B, V, cap, lens, kws, greedy_row, seed):
    """vcla_sample_rows_table over B rows with the records `kws` (row greedy_row flagged greedy) against vcla_sample on every row alone"""
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, V, generator=g) * 3).to(DEV)
    hist = torch.randint(0, 9, (cap, B), generator=g).to(DEV)
    uni = torch.rand(cap, B, generator=g).to(DEV)
    kid = torch.full((B, L.SAMPLE_KEPT_LD), -1, dtype=torch.int64, device=DEV)
    nk = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((B,), -9, dtype=torch.int64, device=DEV)
    rows = L.sample_row_bytes(L.sample_row_table([dict(kw, greedy=(b == greedy_row)) for b, kw in enumerate(kws)])).to(DEV)
    lg = logits.clone()
    L.sample_rows_table(lg, torch.tensor(lens, dtype=torch.int32, device=DEV), L.sample_args(uniforms=uni, history=hist, kept_ids=kid, n_kept=nk), rows, out=out)
    for b, h in enumerate(lens):
        if h < 0:
            assert int(out[b]) == -9 and int(nk[b]) == -1 and torch.equal(lg[b], logits[b]), (seed, b)        # skipped: nothing touched
            continue
        hb = hist[:, b:b + 1].contiguous()
        ub = None if b == greedy_row else uni[:, b:b + 1].contiguous()           # a greedy row draws at 0, which is what no uniforms means
        kid1 = torch.full((1, L.SAMPLE_KEPT_LD), -1, dtype=torch.int64, device=DEV)
        nk1 = torch.zeros(1, dtype=torch.int32, device=DEV)
        lg1 = logits[b:b + 1].clone()
        want = L.sample(lg1, L.sample_args(uniforms=ub, history=hb, kept_ids=kid1, n_kept=nk1, **kws[b]), n_hist=h)
        n = int(nk1[0])
        assert int(out[b]) == int(want[0]) and int(nk[b]) == n and torch.equal(kid[b, :n], kid1[0, :n]), (seed, b, h)
        assert torch.equal(lg[b], lg1[0]), (seed, b, h)          # the penalties and bans written into the row are the same too
        if b == greedy_row:                                       # whatever its uniform is: the first maximum of its processed scores
            assert float(uni[h, b]) > 0 and int(out[b]) == int(L.argmax(lg[b:b + 1])[0]), (seed, b)


def test_sample_rows_table_vs_sample_per_row():
    from tests.test_sampling_oracle import CFGS
    lens = [0, 3, -1, 47, 20, 1, -5]
    for shift in range(len(CFGS)):
        kws = [_kw(CFGS[(b + shift) % len(CFGS)]) for b in range(7)]
        _table_vs_rows(7, 4099, 48, lens, kws, greedy_row=(3, 4, 5, 0, 1)[shift % 5], seed=50 + shift)


def test_sample_rows_table_at_the_register_slice_limit():
    from tests.test_sampling_oracle import CFGS
    L = _lib()
    _table_vs_rows(2, L.SAMPLE_MAX_VOCAB, 8, [5, 0], [_kw(CFGS[0]), _kw(CFGS[1])], greedy_row=-1, seed=7)


def test_sample_rows_table_refuses_null_tables():
    L = _lib()
    lg = torch.zeros(1, 16, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, dtype=torch.int64, device=DEV)
    hist = torch.zeros(1, 1, dtype=torch.int64, device=DEV)
    a = L.sample_args(history=hist)
    with pytest.raises(ValueError, match="rows is NULL"):
        L.check(L.load().vcla_sample_rows_table(lg.data_ptr(), 16, 1, 16, n.data_ptr(), C.byref(a), None, out.data_ptr(), L.stream_ptr()))
    rows = L.sample_row_bytes(L.sample_row_table([{}])).to(DEV)
    with pytest.raises(ValueError, match="n_hist_rows or shared->history is NULL"):
        L.check(L.load().vcla_sample_rows_table(lg.data_ptr(), 16, 1, 16, None, C.byref(a), rows.data_ptr(), out.data_ptr(), L.stream_ptr()))


# ------------------------------------------------------------------ 2. one eos list per slot in the bookkeeping kernel
SLOT_SEED = 23


def _slot_cases(seed=SLOT_SEED, n_cases=60):
    """the cases of the kernel test, and how many rows the host model finishes on an id that is an eos for them but not for some other
    row that was active in the same step"""
    from visualcla import inflight as I
    rng = random.Random(seed)
    cases, own = [], 0
    for _ in range(n_cases):
        B = rng.choice([1, 2, 5, 16, 33, 64, 70])
        cap = rng.randint(2, 12)
        eos_rows = [rng.sample(range(10), rng.randint(0, 8)) for _ in range(B)]
        row_pos = [rng.choice([-1, rng.randint(0, 500)]) for _ in range(B)]
        count = [rng.randint(1, cap - 1) for _ in range(B)]
        budget = [min(cap, c + rng.choice([1, 1, 2, 5])) for c in count]
        cur = [rng.randint(0, 96) for _ in range(B)]
        hist = [[rng.randint(0, 96) for _ in range(B)] for _ in range(cap)]
        ids = [[rng.randint(0, 9) for _ in range(B)] for _ in range(3)]
        cases.append(dict(B=B, cap=cap, eos_rows=eos_rows, row_pos=row_pos, count=count, budget=budget, cur=cur, hist=hist, ids=ids))
        rp, ct, cu, hi = list(row_pos), list(count), list(cur), [list(r) for r in hist]
        for step in ids:
            before = list(rp)
            I.slot_step_model(step, rp, ct, budget, hi, cu, [], eos_rows=eos_rows)
            for b in range(B):
                if before[b] >= 0 and rp[b] < 0 and step[b] in eos_rows[b]:
                    own += any(before[c] >= 0 and step[b] not in eos_rows[c] for c in range(B) if c != b)
    return cases, own


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_slot_step_rows_kernel_vs_host(dt):
    from visualcla import inflight as I
    L = _lib()
    lib = L.load()
    V, D = 97, 64
    table = torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)
    cases, own = _slot_cases()
    assert own >= 20, own                                         # (the host model's count: the seed is chosen so that it holds)
    n_own = 0
    for k, c in enumerate(cases):
        B, eos_rows = c["B"], c["eos_rows"]
        row_pos, count, budget, cur, hist = list(c["row_pos"]), list(c["count"]), c["budget"], list(c["cur"]), [list(r) for r in c["hist"]]
        hl = [n if p >= 0 else -1 for n, p in zip(count, row_pos)]
        st = torch.tensor(row_pos + count + hl + budget + [0] * L.SLOT_SUMMARY_WORDS, dtype=torch.int32, device=DEV)
        hist_t = torch.tensor(hist, dtype=torch.int64, device=DEV)
        cur_t = torch.tensor(cur, dtype=torch.int64, device=DEV)
        x = torch.zeros(B, D, dtype=dt, device=DEV)
        eos_t = L.slot_eos_rows(eos_rows).to(DEV)
        a = L.slot_args([2, 3], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist_t, cur_t, st[4 * B:])       # the shared list is ignored
        for step, ids in enumerate(c["ids"]):
            before = list(row_pos)
            ids_t = torch.tensor(ids, dtype=torch.int64, device=DEV)
            L.check(lib.vcla_slot_step_rows(ids_t.data_ptr(), C.byref(a), eos_t.data_ptr(), table.data_ptr(), x.data_ptr(), D, V, L.dtype_code(dt), L.stream_ptr()))
            n_act = I.slot_step_model(ids, row_pos, count, budget, hist, cur, [2, 3], hl, eos_rows=eos_rows)
            s = st.tolist()
            assert s[:B] == row_pos and s[B:2 * B] == count and s[2 * B:3 * B] == hl and s[3 * B:4 * B] == budget, (k, step)
            assert s[4 * B] == n_act and s[4 * B + 1] == 0, (k, step)
            assert hist_t.tolist() == hist and cur_t.tolist() == cur, (k, step)
            assert torch.equal(x.float(), table[cur_t].float()), (k, step)
            for b in range(B):
                if before[b] >= 0 and s[b] < 0 and ids[b] in eos_rows[b]:
                    n_own += any(before[j] >= 0 and ids[b] not in eos_rows[j] for j in range(B) if j != b)
    assert n_own == own
    # eos_rows NULL: the entry is vcla_slot_step
    st = torch.tensor([4, 4, 1, 1, 1, 1, 9, 9, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    hist_t, cur_t, x = torch.zeros(4, 2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, D, dtype=dt, device=DEV)
    a = L.slot_args([3], st[:2], st[2:4], st[6:8], st[4:6], hist_t, cur_t, st[8:])
    L.check(lib.vcla_slot_step_rows(torch.tensor([3, 5], device=DEV).data_ptr(), C.byref(a), None, table.data_ptr(), x.data_ptr(), D, V, L.dtype_code(dt), L.stream_ptr()))
    assert st.tolist()[:9] == [-1, 5, 2, 2, -1, 2, 9, 9, 1]


# ------------------------------------------------------------------ 3. end to end, fp32, a deterministic mix of four configs
@pytest.fixture(scope="module")
def tiny():
    cfg = O.cfg_tiny()
    W = O.make_weights(cfg, seed=0)
    reqs = _requests(cfg)
    want, margin = _oracle(cfg, W, reqs)
    return cfg, W, reqs, want, margin, make_hip_model(cfg, W, torch.float32)


def _with(reqs, cfgs, seeds=None):
    out = _as_dicts(reqs)
    for i, r in enumerate(out):
        if cfgs is not None and cfgs[i] is not None:
            r["generation_config"] = cfgs[i]
        if seeds is not None and seeds[i] is not None:
            r["seed"] = seeds[i]
    return out


def test_generate_many_mixed_configs_equal_generate_alone_fp32(tiny):
    cfg, W, reqs, want, margin, m = tiny
    print(f"[per-request] smallest top-2 margin over {sum(BUDGETS)} greedy steps = {margin:.3e}")
    assert margin >= 1e-4, f"margin {margin:.2e}: equality of greedy ids is not decidable at these prompt seeds"
    eos1 = sorted({int(want[r][len(want[r]) // 2]) for r in (5, 9)})                  # ids plain greedy produces: they end requests early
    pen = dict(do_sample=True, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=3, min_new_tokens=4)
    plain = m.generate(input_ids=reqs[10][0].cuda(), pixel_values=reqs[10][1].cuda(), max_new_tokens=40, eos_token_id=None, **pen)[0].cpu()
    classes = [dict(do_sample=False, eos_token_id=None), dict(do_sample=False, eos_token_id=eos1), dict(pen, eos_token_id=int(plain[6])),
               dict(do_sample=False, repetition_penalty=1.3, eos_token_id=None)]
    cfgs = [classes[i % 4] for i in range(12)]
    alone = [m.generate(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, **cfgs[i])[0].cpu()
             for i, (ids, px, n) in enumerate(reqs)]
    for i in (0, 4, 8):
        assert torch.equal(alone[i], want[i])
    for i in (1, 5, 9):
        assert torch.equal(alone[i], _cut(want[i], eos1))
    assert sum(len(a) < n for a, (_, _, n) in zip(alone, reqs)) >= 3              # requests do end early, on their own eos
    assert any(not torch.equal(alone[i], want[i][:len(alone[i])]) for i in (3, 7, 11))      # the penalty of class 3 does change ids

    def check(got, tag):
        for i in range(12):
            assert torch.equal(got[i].cpu(), alone[i]), (tag, i, got[i].tolist(), alone[i].tolist())
    for sps in (2, 8):
        check(m.generate_many(_with(reqs, cfgs), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=None), sps)
        st = m.last_inflight_stats
        assert st["config_classes"] == 4 and st["sampler_rows"] == 6 and st["seeded"] == 0 and st["slots"] == 4
        assert st["tokens"] == sum(len(a) for a in alone)
    check(m.generate_many(_with(reqs, cfgs), max_batch=4, steps_per_sync=3, use_graph=False, do_sample=False, eos_token_id=None), "eager")
    check(m.generate_many(_with(reqs, cfgs), max_batch=4, steps_per_sync=3, share_prefix=True, do_sample=False, eos_token_id=None), "share_prefix")
    rev = m.generate_many(_with(reqs, cfgs)[::-1], max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=None)
    check(rev[::-1], "reversed")
    # GenerationConfig objects instead of dicts
    from transformers import GenerationConfig
    check(m.generate_many(_with(reqs, [GenerationConfig(**c) for c in cfgs]), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=None), "objects")
    assert m.last_inflight_stats["config_classes"] == 4
    # greedy requests that differ in their eos only: argmax and the per-row eos lookup, no sampler
    g2 = [classes[i % 2] for i in range(12)]
    got = m.generate_many(_with(reqs, g2), max_batch=4, steps_per_sync=3, do_sample=True, top_k=5)
    assert m.last_inflight_stats["config_classes"] == 2 and m.last_inflight_stats["sampler_rows"] == 0
    for i in range(12):
        assert torch.equal(got[i].cpu(), want[i] if i % 2 == 0 else _cut(want[i], eos1)), i
    # one config given per request, the same for all: the uniform route, and the queue-level call's results
    same = m.generate_many(_with(reqs, [classes[2]] * 12), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=None)
    st1 = dict(m.last_inflight_stats)
    queue = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=3, **classes[2])
    st2 = m.last_inflight_stats
    assert st1["config_classes"] == st2["config_classes"] == 1 and st1["sampler_rows"] == st2["sampler_rows"] == 12
    assert st1["steps"] == st2["steps"] and all(torch.equal(a, b) for a, b in zip(same, queue))
    # refusals name the requests, in one message, before anything runs
    bad = list(cfgs)
    bad[3], bad[7] = dict(num_beams=2), dict(do_sample=True, typical_p=0.5)
    with pytest.raises(ValueError) as e:
        m.generate_many(_with(reqs, bad), max_batch=4, do_sample=False, eos_token_id=None)
    assert "request 3: num_beams=2" in str(e.value) and "request 7: typical_p=0.5" in str(e.value)


# ------------------------------------------------------------------ 4. end to end, fp32, seeded sampling
SAMPLING = [dict(temperature=0.7, top_k=40, top_p=0.9), dict(temperature=1.0, top_k=50, top_p=0.95), dict(temperature=0.5, top_k=5, top_p=1.0)]


def test_generate_many_seeded_sampling_fp32(tiny):
    cfg, W, reqs, want, margin, m = tiny
    seeds = [100 + i for i in range(12)]
    cfgs = [dict(do_sample=True, eos_token_id=None, **SAMPLING[i % 3]) for i in range(12)]
    torch.manual_seed(1)
    mixed = m.generate_many(_with(reqs, cfgs, seeds), max_batch=4, steps_per_sync=4, do_sample=False, eos_token_id=None)
    st = m.last_inflight_stats
    assert st["config_classes"] == 3 and st["sampler_rows"] == 12 and st["seeded"] == 12 and [len(x) for x in mixed] == BUDGETS
    torch.manual_seed(2)                                          # the default generator plays no part for seeded requests
    again = m.generate_many(_with(reqs, cfgs, seeds), max_batch=4, steps_per_sync=4, do_sample=False, eos_token_id=None)
    assert all(torch.equal(a, b) for a, b in zip(mixed, again))
    differ = 0
    for c in range(3):
        # the same queue -- seeds, budgets, slots, schedule (nothing ends early) -- under class c as the one config of the queue
        uniform = m.generate_many(_with(reqs, None, seeds), max_batch=4, steps_per_sync=4, do_sample=True, eos_token_id=None, **SAMPLING[c])
        assert m.last_inflight_stats["config_classes"] == 1 and m.last_inflight_stats["seeded"] == 12
        for i in range(12):
            if i % 3 == c:
                assert torch.equal(mixed[i], uniform[i]), (c, i, mixed[i].tolist(), uniform[i].tolist())
            else:
                differ += not torch.equal(mixed[i], uniform[i])
    assert differ >= 6                                            # the classes are different samplers: the comparison above is no tautology
    assert sum(not torch.equal(a.cpu(), b[:len(a)]) for a, b in zip(mixed, want)) >= 6      # ... and the draws are no greedy decoding
    # the one-slot route honours both keys: a seed changes nothing where nothing is drawn (top_k = 1) ...
    k1 = dict(do_sample=True, top_k=1, temperature=0.7, eos_token_id=None)
    a = m.generate_many(_with(reqs[9:11], [k1, k1], [5, 6]), max_batch=1, do_sample=False, eos_token_id=None)
    b = m.generate_many(_with(reqs[9:11], [k1, k1]), max_batch=1, do_sample=False, eos_token_id=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x.cpu(), y) for x, y in zip(a, want[9:11]))
    assert m.last_inflight_stats["slots"] == 1 and m.last_inflight_stats["config_classes"] == 1
    # ... and makes a sampled request reproducible there too, under its own config
    c1 = m.generate_many(_with(reqs[9:11], cfgs[9:11], [5, 6]), max_batch=1, do_sample=False, eos_token_id=None)
    torch.manual_seed(3)
    c2 = m.generate_many(_with(reqs[9:11], cfgs[9:11], [5, 6]), max_batch=1, do_sample=False, eos_token_id=None)
    assert all(torch.equal(x, y) for x, y in zip(c1, c2)) and [len(x) for x in c1] == BUDGETS[9:11]
    assert m._request_seed is None


# ------------------------------------------------------------------ 5. bf16 / W8A16 at the LLaMA-7B widths
@pytest.mark.parametrize("fp8", [False, True])
def test_generate_many_mixed_configs_bf16_engine_widths(fp8):
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=1024))
    m = make_hip_model(cfg, O.make_weights(cfg, seed=2), torch.bfloat16)
    if fp8:
        m.enable_fp8_decode(True, prefill=False)
    g = torch.Generator().manual_seed(1)
    rng = random.Random(4)
    reqs = [(torch.randint(3, 4000, (1, rng.randint(20, 90)), generator=g), None, 12) for _ in range(8)]      # equal budgets: one slot schedule for every run
    seeds = [40 + i for i in range(8)]
    greedy, sampled = dict(do_sample=False, eos_token_id=None), dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.9, eos_token_id=None)
    cfgs = [greedy if i % 2 == 0 else sampled for i in range(8)]
    mixed = m.generate_many(_with(reqs, cfgs, seeds), max_batch=4, steps_per_sync=4, do_sample=False, eos_token_id=None)
    assert m.last_inflight_stats["config_classes"] == 2 and m.last_inflight_stats["sampler_rows"] == 4 and [len(x) for x in mixed] == [12] * 8
    for c, kw in enumerate((greedy, sampled)):
        uniform = m.generate_many(_with(reqs, None, seeds), max_batch=4, steps_per_sync=4, **kw)
        for i in range(8):
            if i % 2 == c:
                assert torch.equal(mixed[i], uniform[i]), (c, i, mixed[i].tolist(), uniform[i].tolist())
    assert any(not torch.equal(mixed[i], uniform[i]) for i in range(0, 8, 2))     # (uniform: the sampled run) greedy rows are not sampled rows


# ------------------------------------------------------------------ 6. chat_many with one config / seed per item
from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_many_per_item_configs_equal_chat(loaded, capsys):  # noqa: F811
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    img = _image()
    texts = ["what is this?", "hello world", "a cat sitting on a mat", "describe the image", "tiny corpus"]

    def queue_gc():
        return GenerationConfig(max_new_tokens=7, do_sample=False, eos_token_id=None)

    def own(k):                                                   # (config given to chat_many, the config chat() gets for the same item)
        if k == 1:
            return (GenerationConfig(max_new_tokens=5, do_sample=False, repetition_penalty=1.3),) * 2
        if k == 2:
            return dict(no_repeat_ngram_size=2), GenerationConfig(max_new_tokens=7, do_sample=False, eos_token_id=None, no_repeat_ngram_size=2)
        if k == 4:
            return (GenerationConfig(max_new_tokens=6, do_sample=True, top_k=1, repetition_penalty=1.2),) * 2
        return None, queue_gc()

    def history(k):
        return [] if k != 2 else [{"type": "instruction", "value": "hello", "first_instruction": True}, {"type": "response", "value": "a cat"}]
    want = [visualcla.chat(model, img, text, history=history(k), generation_config=own(k)[1]) for k, text in enumerate(texts)]
    capsys.readouterr()
    items = [(img, text) if k != 2 else (img, text, history(k)) for k, text in enumerate(texts)]
    got = visualcla.chat_many(model, items, generation_config=queue_gc(), max_batch=3, generation_configs=[own(k)[0] for k in range(5)],
                              seeds=[None, None, None, None, 9])
    st = model.last_inflight_stats
    assert st["config_classes"] == 4 and st["seeded"] == 1 and st["sampler_rows"] == 3
    assert len(got) == len(want)
    for (r1, h1), (r2, h2) in zip(want, got):
        assert r1 == r2 and h1 == h2
    assert got[2][1] is items[2][2] and len(got[2][1]) == 4
    plain = visualcla.chat_many(model, [(img, text) for text in texts], generation_config=queue_gc(), max_batch=3)
    assert any(a[0] != b[0] for a, b in zip(plain, got))          # the items' own configs did change responses

"""Prompt-lookup decoding on the GPU: the verify attention kernel (vcla_attn_verify) against fp32 torch and against R sequential decode steps,
the draft/accept kernel (vcla_lookup_step) against the host restatement, and generate(prompt_lookup_num_tokens=k) against plain greedy."""
import ctypes as C
import dataclasses
import os
import random
import subprocess
import sys

import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from visualcla import _lib as L
    return L


# ------------------------------------------------------------------ 1. verify attention
def _rope_ref(x, cos, sin, dt):
    """rotate-half RoPE with the kernels' roundings: x [R, H, d] fp32 (dtype values), cos / sin [R, d/2]"""
    h = x.shape[-1] // 2
    c = cos.to(dt).float()[:, None, :]
    s = sin.to(dt).float()[:, None, :]
    a, b = x[..., :h], x[..., h:]
    return torch.cat([(a * c - b * s).to(dt).float(), (b * c + a * s).to(dt).float()], dim=-1)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("R", [2, 5, 8, 16])
def test_verify_attention_vs_torch_and_decode(dt, d, masked, R):
    L = _lib()
    lib = L.load()
    dev = "cuda"
    H, ctx_max = 4, 2048
    code = L.dtype_code(dt)
    g = torch.Generator(device="cpu").manual_seed(R * 7 + d + masked)
    ang = torch.rand(ctx_max, d // 2, generator=g) * 6.28
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    for ctx in (1, 37, 509, 700, 1900):
        kv = (torch.randn(2, H, ctx_max, d, generator=g) * 0.5).to(dt).to(dev)
        qkv = torch.randn(R, 3 * H * d, generator=g).to(dt).to(dev)
        km = None
        if masked:
            km = torch.ones(1, ctx_max, dtype=torch.int32)
            km[0, :ctx] = (torch.rand(ctx, generator=g) > 0.3).int()
            km = km.to(dev)
        scale = d ** -0.5
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.zeros(R, H * d, dtype=dt, device=dev)
        kv_v = kv.clone()
        nb = lib.vcla_attn_verify_scratch_bytes(H, d, ctx_max)
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        L.check(lib.vcla_attn_verify(qkv.data_ptr(), kv_v[0].data_ptr(), kv_v[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), R, H, d,
                                     ctx_max, ctx, pos_dev.data_ptr(), L.ptr(km), scale, code, 0, scratch.data_ptr(), scratch.numel(), L.stream_ptr()))
        # R sequential decode steps write the same K / V rows, bitwise
        kv_d = kv.clone()
        o1 = torch.zeros(1, H * d, dtype=dt, device=dev)
        for r in range(R):
            L.check(lib.vcla_attn_decode_fused(qkv[r:r + 1].contiguous().data_ptr(), kv_d[0].data_ptr(), kv_d[1].data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                               o1.data_ptr(), 1, H, d, ctx_max, ctx + r, None, L.ptr(km), ctx_max, scale, code, 0, L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(kv_v, kv_d), f"ctx {ctx}: appended rows differ from the decode kernel's"
        # fp32 attention over the same cache
        q = _rope_ref(qkv[:, :H * d].float().view(R, H, d), cos[ctx:ctx + R], sin[ctx:ctx + R], dt)
        K, V = kv_v[0].float(), kv_v[1].float()
        s = torch.einsum("rhd,hjd->rhj", q, K[:, :ctx + R]) * scale
        j = torch.arange(ctx + R, device=dev)
        vis = j[None, :] <= (ctx + torch.arange(R, device=dev))[:, None]
        if km is not None:
            vis = vis & (km[0, :ctx + R] != 0)[None, :]
        s = s.masked_fill(~vis[:, None, :], float("-inf"))
        p = torch.softmax(s, dim=-1).nan_to_num(0.0)
        ref = torch.einsum("rhj,hjd->rhd", p, V[:, :ctx + R]).reshape(R, H * d)
        tol = 2e-2 if dt == torch.bfloat16 else 1e-4
        err = (out.float() - ref).abs().max().item()
        assert err < tol, f"ctx {ctx}: max |err| {err}"


def test_verify_attention_fragment_output():
    L = _lib()
    lib = L.load()
    dev, dt, H, d, R, ctx_max, ctx = "cuda", torch.bfloat16, 8, 128, 7, 1024, 600
    g = torch.Generator(device="cpu").manual_seed(3)
    ang = torch.rand(ctx_max, d // 2, generator=g)
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    kv = torch.randn(2, H, ctx_max, d, generator=g).to(dt).to(dev)
    qkv = torch.randn(R, 3 * H * d, generator=g).to(dt).to(dev)
    scratch = torch.empty(lib.vcla_attn_verify_scratch_bytes(H, d, ctx_max), dtype=torch.uint8, device=dev)
    outs = []
    for frag in (0, 1):
        o = torch.zeros(16 * H * d if frag else R * H * d, dtype=dt, device=dev)
        k2 = kv.clone()
        L.check(lib.vcla_attn_verify(qkv.data_ptr(), k2[0].data_ptr(), k2[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), o.data_ptr(), R, H, d, ctx_max,
                                     ctx, None, None, d ** -0.5, L.VCLA_BF16, frag, scratch.data_ptr(), scratch.numel(), L.stream_ptr()))
        outs.append(o)
    r = torch.arange(R, device=dev)[:, None]
    k = torch.arange(H * d, device=dev)[None, :]
    idx = (((k >> 5) * 64 + ((k & 31) >> 3) * 16 + r) << 3) + (k & 7)
    assert torch.equal(outs[1][idx], outs[0].view(R, H * d))


# ------------------------------------------------------------------ 2. draft / accept kernel
def test_lookup_step_kernel_vs_host():
    from visualcla import prompt_lookup as PL
    L = _lib()
    lib = L.load()
    dev = "cuda"
    rng = random.Random(11)
    n_eos_hit = n_budget = n_acc = 0
    for case in range(120):
        k = rng.randint(1, 15)
        ngram = rng.randint(1, 3)
        eos = rng.choice([[], [2], [2, 3]])
        budget = rng.randint(1, 30)
        hist0 = [rng.randint(0, 6) for _ in range(rng.randint(2, 40))]
        cap = len(hist0) + budget + 1
        hist_t = torch.zeros(cap, dtype=torch.int64, device=dev)
        hist_t[:len(hist0)] = torch.tensor(hist0, device=dev)
        out_t = torch.zeros(budget, dtype=torch.int64, device=dev)
        row_t = torch.zeros(k + 1, dtype=torch.int64, device=dev)
        state = torch.zeros(L.LOOKUP_STATE_WORDS, dtype=torch.int32, device=dev)
        state[L.LOOKUP_NHIST] = len(hist0)
        pos = torch.zeros(1, dtype=torch.int32, device=dev)
        a = L.lookup_args(k, ngram, budget, eos, row_t, hist_t, out_t, state)
        L.check(lib.vcla_lookup_step(None, C.byref(a), pos.data_ptr(), L.stream_ptr()))
        hist, out = list(hist0), []
        st = dict(done=0, pos=0, iterations=0, accepted=0)
        row = PL.next_row(hist, k, ngram, eos)
        assert row_t.tolist() == row, case
        for it in range(12):
            # argmax: follow the drafts for a while, then diverge; sometimes an eos
            n_follow = rng.randint(0, k)
            am = [row[i + 1] if i < n_follow else rng.randint(0, 6) for i in range(k)] + [rng.randint(0, 6)]
            am_t = torch.tensor(am, dtype=torch.int64, device=dev)
            L.check(lib.vcla_lookup_step(am_t.data_ptr(), C.byref(a), pos.data_ptr(), L.stream_ptr()))
            was_done = st["done"]
            row = PL.lookup_step(row, am, hist, out, st, budget, eos, k, ngram)
            s = state.tolist()
            assert out_t[:s[L.LOOKUP_COUNT]].tolist() == out and s[L.LOOKUP_DONE] == st["done"], (case, it)
            assert int(pos.item()) == st["pos"] and s[L.LOOKUP_ACCEPTED] == st["accepted"], (case, it)
            assert hist_t[:s[L.LOOKUP_NHIST]].tolist() == hist and row_t.tolist() == row, (case, it)
            if st["done"] and not was_done:
                n_eos_hit += bool(out and out[-1] in eos)
                n_budget += len(out) == budget
            n_acc += st["accepted"] > 0
    assert n_eos_hit > 5 and n_budget > 5 and n_acc > 20


# ------------------------------------------------------------------ 3. exactness, fp32
def _text_ids(cfg, T, seed):
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)       # ordinary ids below the image specials
    return torch.randint(3, hi, (1, T), generator=torch.Generator().manual_seed(seed))


def _repetitive_ids(cfg, T, seed, with_image):
    if with_image:
        px, ids, _ = O.make_inputs(cfg, 1, T, seed_ids=seed)
    else:
        px, ids = None, _text_ids(cfg, T, seed)
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    g = torch.Generator().manual_seed(seed)
    phrase = torch.randint(3, hi, (7,), generator=g)
    tail = phrase.repeat(6)
    ids = torch.cat([ids, tail[None]], dim=1)
    return (px if with_image else None), ids


def _random_ids(cfg, T, seed):
    return None, _text_ids(cfg, T, seed)


@pytest.fixture(scope="module")
def tiny32():
    cfg = O.cfg_tiny()
    return cfg, make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)


@pytest.fixture(scope="module")
def small32():
    cfg = O.cfg_small()
    return cfg, make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)


def _pair(m, px, ids, n, k, eos=None, **kw):
    base = dict(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, do_sample=False, eos_token_id=eos, **kw)
    plain = m.generate(**base).cpu()
    look = m.generate(prompt_lookup_num_tokens=k, **base).cpu()
    return plain, look


@pytest.mark.parametrize("which", ["tiny32", "small32"])
@pytest.mark.parametrize("k", [1, 3, 7, 15])
def test_lookup_generate_equals_greedy_fp32(which, k, request):
    cfg, m = request.getfixturevalue(which)
    px, ids = _repetitive_ids(cfg, 40, 5, with_image=True)
    plain, look = _pair(m, px, ids, 48, k)
    assert torch.equal(plain, look)
    assert m.last_lookup_stats["accepted"] >= 1, m.last_lookup_stats
    assert m.last_lookup_stats["iterations"] < 47
    # eos respected: the token plain greedy produces at step 9 as the eos id
    eos = int(plain[0, 9])
    plain_e, look_e = _pair(m, px, ids, 48, k, eos=eos)
    assert torch.equal(plain_e, look_e) and int(look_e[0, -1]) == eos
    # a random (non-repeating) prompt, no image
    px2, ids2 = _random_ids(cfg, 30, 9)
    plain2, look2 = _pair(m, None, ids2, 25, k)
    assert torch.equal(plain2, look2)


def test_lookup_generate_budget_edges(tiny32):
    cfg, m = tiny32
    px, ids = _repetitive_ids(cfg, 40, 6, with_image=False)
    for n in (1, 2, 3):
        plain, look = _pair(m, None, ids, n, 4)
        assert torch.equal(plain, look) and look.shape == (1, n)
    # k shrinks to fit max_position_embeddings; 0 falls back to plain greedy
    T = ids.shape[1]
    n = cfg.text.max_position_embeddings - T - 2
    plain, look = _pair(m, None, ids, n, 7)
    assert torch.equal(plain, look)
    n = cfg.text.max_position_embeddings - T
    plain, look = _pair(m, None, ids, n, 7)
    assert torch.equal(plain, look)


# ------------------------------------------------------------------ 4. bf16 / fp8 decode weights, LLaMA-7B widths
def _teacher_forced_check(m, ids, toks, plain):
    full = torch.cat([ids, toks[:, :-1]], dim=1).cuda()
    lg = m(input_ids=full).logits[0].float()
    T = ids.shape[1]
    rows = lg[T - 1:T - 1 + toks.shape[1]]
    top2 = rows.topk(2, dim=-1)
    gap = (top2.values[:, 0] - top2.values[:, 1]).cpu()
    am = rows.argmax(dim=-1).cpu()
    clear = gap >= 0.05
    assert torch.equal(am[clear], toks[0][clear]), (am, toks)
    first_tie = int((~clear).nonzero()[0]) if (~clear).any() else toks.shape[1]
    n = min(first_tie, plain.shape[1], toks.shape[1])
    assert torch.equal(plain[0, :n], toks[0, :n])


def _greedy_step_gaps(m, ids, n):
    """plain greedy through the host-driven step path (the decode kernels of the fast loop): its tokens and each step's top-2 logit gap"""
    from transformers import LogitsProcessorList
    seen = []

    def grab(i, s):
        seen.append(s.detach().float().cpu().clone())
        return s
    toks = m.generate(input_ids=ids.cuda(), max_new_tokens=n, do_sample=False, eos_token_id=None, logits_processor=LogitsProcessorList([grab])).cpu()
    sc = torch.cat(seen)
    top2 = sc.topk(2, dim=-1).values
    return toks, (top2[:, 0] - top2[:, 1])


@pytest.mark.parametrize("fp8", [False, True])
def test_lookup_bf16_engine_widths(fp8):
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=1024))
    m = make_hip_model(cfg, O.make_weights(cfg, seed=2), torch.bfloat16)
    if fp8:
        m.enable_fp8_decode(True, prefill=False)
    g = torch.Generator().manual_seed(1)
    phrase = torch.randint(3, 4000, (11,), generator=g)
    ids = torch.cat([torch.randint(3, 4000, (400,), generator=g), phrase.repeat(10)])[None]      # 510 tokens: the decode crosses 512 keys
    for k in (2, 5):
        base = dict(input_ids=ids.cuda(), max_new_tokens=40, do_sample=False, eos_token_id=None)
        plain = m.generate(**base).cpu()
        look = m.generate(prompt_lookup_num_tokens=k, **base).cpu()
        assert look.shape == plain.shape
        if not fp8:
            _teacher_forced_check(m, ids, look, plain)
        else:
            # forward() runs the bf16 weights (the fp8 copies serve decode steps only): the reference is the greedy step path itself,
            # exact up to the first near-tie of its own logits
            steps, gap = _greedy_step_gaps(m, ids, 40)
            first_tie = int((gap < 0.05).nonzero()[0]) if bool((gap < 0.05).any()) else 40
            assert torch.equal(look[0, :first_tie], steps[0, :first_tie]) and torch.equal(plain[0, :first_tie], steps[0, :first_tie])


# ------------------------------------------------------------------ 5. graph vs eager, graph slots
def test_lookup_graph_vs_eager(tiny32):
    cfg, m = tiny32
    px, ids = _repetitive_ids(cfg, 40, 7, with_image=True)
    kw = dict(input_ids=ids.cuda(), pixel_values=px.cuda(), max_new_tokens=40, do_sample=False, eos_token_id=None, prompt_lookup_num_tokens=4)
    a = m.generate(use_graph=True, **kw).cpu()
    b = m.generate(use_graph=False, **kw).cpu()
    c = m.generate(use_graph=True, **kw).cpu()
    assert torch.equal(a, b) and torch.equal(a, c)


_CHILD = r"""
import sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/visual-chinese-llama-alpaca_amd']
from oracle import visualcla_oracle as O
from tests.helpers import make_hip_model
cfg = O.cfg_tiny()
m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
ids = torch.randint(3, 300, (1, 30), generator=torch.Generator().manual_seed(0)).cuda()
kw = dict(input_ids=ids, max_new_tokens=24, do_sample=False, eos_token_id=None)
tag = lambda s: (print('@@' + s, file=sys.stderr, flush=True))
tag('plain1'); p1 = m.generate(**kw)
tag('look1'); l1 = m.generate(prompt_lookup_num_tokens=3, **kw)
tag('look2'); l2 = m.generate(prompt_lookup_num_tokens=3, **kw)
tag('plain2'); p2 = m.generate(**kw)
torch.cuda.synchronize()
assert torch.equal(p1, l1) and torch.equal(l1, l2) and torch.equal(p1, p2)
tag('end')
"""


def test_lookup_graph_slot_keeps_decode_graph():
    env = dict(os.environ, VCLA_MACRO_GRAPH_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    parts = {}
    cur = None
    for line in r.stderr.splitlines():
        if line.startswith("@@"):
            cur = line[2:]
            parts[cur] = []
        elif cur:
            parts[cur].append(line)
    seg = {k_: "\n".join(v) for k_, v in parts.items()}
    assert "lookup graph" in seg["look1"] and "capture" in seg["look1"]
    look2 = [ln for ln in seg["look2"].splitlines() if "lookup graph" in ln]
    assert look2 and all("replay" in ln for ln in look2)
    assert "decode graph" in seg["plain2"] and "replay" in seg["plain2"]
    assert "decode graph" not in seg["look1"] + seg["look2"]


# ------------------------------------------------------------------ 6. refusals by name
def test_lookup_refusals(tiny32):
    from transformers import StoppingCriteriaList
    cfg, m = tiny32
    ids = torch.randint(3, 300, (1, 20), generator=torch.Generator().manual_seed(0)).cuda()
    base = dict(max_new_tokens=5, eos_token_id=None)
    cases = [
        (dict(input_ids=ids.repeat(2, 1), prompt_lookup_num_tokens=3), "batch size"),
        (dict(input_ids=ids, prompt_lookup_num_tokens=3, num_beams=2), "num_beams"),
        (dict(input_ids=ids, prompt_lookup_num_tokens=3, do_sample=True), "do_sample"),
        (dict(input_ids=ids, prompt_lookup_num_tokens=3, repetition_penalty=1.2), "repetition_penalty"),
        (dict(input_ids=ids, prompt_lookup_num_tokens=3, stopping_criteria=StoppingCriteriaList([lambda i, s, **k: False])), "stopping_criteria"),
        (dict(input_ids=ids, prompt_lookup_num_tokens=16), "prompt_lookup_num_tokens"),
    ]
    for kw, word in cases:
        with pytest.raises(ValueError, match=word) as e:
            m.generate(**base, **kw)
        assert "prompt_lookup_num_tokens" in str(e.value)


def test_lookup_refuses_e4m3_cache():
    cfg = cfg_engine_small()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=3), torch.bfloat16)
    m.enable_fp8_decode(True, prefill=False, kv_cache=True)
    ids = torch.randint(3, 4000, (1, 20), generator=torch.Generator().manual_seed(0)).cuda()
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens.*e4m3"):
        m.generate(input_ids=ids, max_new_tokens=5, eos_token_id=None, prompt_lookup_num_tokens=3)


# ------------------------------------------------------------------ 7. soak
def test_lookup_soak_fp32(tiny32):
    cfg, m = tiny32
    rng = random.Random(5)
    for i in range(20):
        k = rng.randint(1, 15)
        T = rng.randint(5, 60)
        n = rng.randint(1, 60)
        if rng.random() < 0.5:
            _, ids = _repetitive_ids(cfg, T, 100 + i, with_image=False)
        else:
            _, ids = _random_ids(cfg, T, 100 + i)
        eos = rng.choice([None, 2])
        plain, look = _pair(m, None, ids, n, k, eos=eos, max_matching_ngram_size=rng.randint(1, 3))
        assert torch.equal(plain, look), (i, k, T, n)

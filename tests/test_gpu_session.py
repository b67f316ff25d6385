"""Chat sessions on the MI355X: vcla_attn_extend against arithmetic, vcla_llama_extend against the prefill pair, generate(session=) /
chat(session=) against the same calls without a session and against the CPU oracle."""
import dataclasses

import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CTX = 2048


def _lib():
    from visualcla import _lib as L
    return L


# ------------------------------------------------------------------ 1. the kernel against arithmetic
def _rope_ref(x, cos, sin):
    """rotate-half RoPE with the kernels' bf16 roundings: x [R, H, d] fp32 (bf16 values), cos / sin [R, d/2]"""
    dt = torch.bfloat16
    h = x.shape[-1] // 2
    c = cos.to(dt).float()[:, None, :]
    s = sin.to(dt).float()[:, None, :]
    a, b = x[..., :h], x[..., h:]
    return torch.cat([(a * c - b * s).to(dt).float(), (b * c + a * s).to(dt).float()], dim=-1)


def _from_frag(o, R, HD):
    MT = (R + 15) // 16
    r = torch.arange(R, device=o.device)[:, None]
    k = torch.arange(HD, device=o.device)[None, :]
    idx = ((((k >> 5) * MT + (r >> 4)) * 64 + ((k & 31) >> 3) * 16 + (r & 15)) << 3) + (k & 7)
    return o[idx]


def _extend(qkv, kv, cos, sin, R, H, d, p, frag=0):
    """-> (out [R, H d] bf16, scratch bytes of the call); kv [2, H, CTX, d] is updated in place"""
    L = _lib()
    lib = L.load()
    nb = lib.vcla_attn_extend_scratch_bytes(R, H, d, p)
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    rows = (R + 15) // 16 * 16 if frag else R
    out = torch.zeros(rows * H * d, dtype=torch.bfloat16, device=DEV)
    L.check(lib.vcla_attn_extend(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), R, H, d, CTX, p,
                                 d ** -0.5, L.VCLA_BF16, frag, scratch.data_ptr(), scratch.numel(), L.stream_ptr()))
    return (_from_frag(out, R, H * d) if frag else out.view(R, H * d)), nb


def _attention_ref(qkv, kv_after, cos, sin, R, H, d, p):
    """fp32 attention from the same bf16 inputs: rotated q against the cache as it stands after the append"""
    q = _rope_ref(qkv[:, :H * d].float().view(R, H, d), cos[p:p + R], sin[p:p + R])
    K, V = kv_after[0, :, :p + R].float(), kv_after[1, :, :p + R].float()
    s = torch.einsum("rhd,hjd->rhj", q, K) * d ** -0.5
    vis = torch.arange(p + R, device=DEV)[None, :] <= (p + torch.arange(R, device=DEV))[:, None]
    s = s.masked_fill(~vis[:, None, :], float("-inf"))
    return torch.einsum("rhj,hjd->rhd", torch.softmax(s, dim=-1), V).reshape(R, H * d)


@pytest.mark.parametrize("H", [32, 3])
def test_attn_extend_vs_arithmetic(H):
    """outputs within atol 1.5e-2 of fp32 attention on randn inputs (the bound of test_attention_mfma / test_attn_decode_fused); the appended K / V
    rows bitwise vcla_rope_kv_append's from the same qkv; every other cache row untouched; row-major and fragment-major outputs the same bits"""
    L = _lib()
    lib = L.load()
    d = 128
    g = torch.Generator().manual_seed(40 + H)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(CTX, d, 10000.0))
    kv0 = torch.randn(2, H, CTX, d, generator=g).to(torch.bfloat16).to(DEV)
    splits = qtiles = 0
    worst = 0.0
    for R in (1, 7, 16, 17, 33, 64, 100, 256):
        for p in (0, 1, 63, 200, 511, 512, 1000, 1900):
            if p + R > CTX:
                continue
            qkv = torch.randn(R, 3 * H * d, generator=g).to(torch.bfloat16).to(DEV)
            kv = kv0.clone()
            out, nb = _extend(qkv, kv, cos, sin, R, H, d, p)
            splits += nb > 0
            qtiles += R > L.EXTEND_QTILE_ROWS
            # the pair the prefill launches: RoPE + append from the same qkv
            kv_ref, q2 = kv0.clone(), qkv.clone()
            L.check(lib.vcla_rope_kv_append(q2.data_ptr(), kv_ref[0].data_ptr(), kv_ref[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, R, H, d, CTX, p,
                                            None, L.VCLA_BF16, L.stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(kv[:, :, p:p + R], kv_ref[:, :, p:p + R]), f"R {R} p {p}: appended rows differ from vcla_rope_kv_append's"
            assert torch.equal(kv[:, :, :p], kv0[:, :, :p]) and torch.equal(kv[:, :, p + R:], kv0[:, :, p + R:]), f"R {R} p {p}: rows outside the block changed"
            ref = _attention_ref(qkv, kv, cos, sin, R, H, d, p)
            err = (out.float() - ref).abs().max().item()
            worst = max(worst, err)
            print(f"[attn_extend] H {H} R {R} p {p}: scratch {nb} B, max |err| {err:.3e}")
            assert err < 1.5e-2, f"R {R} p {p}: max |err| {err}"
            if R <= 64:
                kv_f = kv0.clone()
                out_f, _ = _extend(qkv, kv_f, cos, sin, R, H, d, p, frag=1)
                assert torch.equal(out_f, out) and torch.equal(kv_f, kv), f"R {R} p {p}: the fragment-major output differs"
    print(f"[attn_extend] H {H}: worst max |err| {worst:.3e}; {splits} cases with several splits, {qtiles} with several q-tiles")
    assert splits >= 1 and qtiles >= 1      # the merge launch and the q-tile index are not covered by accident


def test_attn_extend_head_dim_64():
    """the d = 64 instantiations (both q-tile sizes, one split and several): same three claims"""
    L = _lib()
    lib = L.load()
    H, d = 5, 64
    g = torch.Generator().manual_seed(64)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(CTX, d, 10000.0))
    kv0 = torch.randn(2, H, CTX, d, generator=g).to(torch.bfloat16).to(DEV)
    for R, p in ((1, 0), (7, 30), (33, 63), (64, 700), (100, 1), (256, 1500)):
        qkv = torch.randn(R, 3 * H * d, generator=g).to(torch.bfloat16).to(DEV)
        kv = kv0.clone()
        out, nb = _extend(qkv, kv, cos, sin, R, H, d, p)
        kv_ref, q2 = kv0.clone(), qkv.clone()
        L.check(lib.vcla_rope_kv_append(q2.data_ptr(), kv_ref[0].data_ptr(), kv_ref[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, R, H, d, CTX, p,
                                        None, L.VCLA_BF16, L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(kv, kv_ref), f"R {R} p {p}: the cache differs from vcla_rope_kv_append's"
        err = (out.float() - _attention_ref(qkv, kv, cos, sin, R, H, d, p)).abs().max().item()
        print(f"[attn_extend d64] R {R} p {p}: scratch {nb} B, max |err| {err:.3e}")
        assert err < 1.5e-2, f"R {R} p {p}: max |err| {err}"
        if R <= 64:
            kv_f = kv0.clone()
            out_f, _ = _extend(qkv, kv_f, cos, sin, R, H, d, p, frag=1)
            assert torch.equal(out_f, out) and torch.equal(kv_f, kv)


def test_attn_extend_planted_key():
    """one key made to matter (value row 100, score 0 -> weight ~ 1 / (1.65 n)): a key dropped or misplaced at a tile seam, a split seam or the
    cache / new-row seam moves the rows that may see it far outside the bound, and a key seen too early moves rows that must not see it"""
    L = _lib()
    H, d, R, p = 3, 128, 40, 700
    g = torch.Generator().manual_seed(77)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(CTX, d, 10000.0))
    kv0 = torch.randn(2, H, CTX, d, generator=g).to(torch.bfloat16).to(DEV)
    qkv0 = torch.randn(R, 3 * H * d, generator=g).to(torch.bfloat16).to(DEV)
    base, nb = _extend(qkv0, kv0.clone(), cos, sin, R, H, d, p)
    assert nb > 0
    S = nb // (H * 64 * (d + 4) * 4)                       # splits of this call: one q-tile of 64 rows
    per = ((p + R + 63) // 64 + S - 1) // S * 64           # keys per split
    assert S > 1
    for j in (0, 63, 64, per - 1, per, 2 * per - 1, 2 * per, p - 1, p, p + 20, p + R - 1):
        kv, qkv = kv0.clone(), qkv0.clone()
        if j < p:
            kv[0, :, j] = 0
            kv[1, :, j] = 100.0
        else:
            qkv.view(R, 3, H, d)[j - p, 1] = 0
            qkv.view(R, 3, H, d)[j - p, 2] = 100.0
        out, _ = _extend(qkv, kv, cos, sin, R, H, d, p)
        ref = _attention_ref(qkv, kv, cos, sin, R, H, d, p)
        first = max(0, j - p)                             # the first row that may see key j
        err = (out.float() - ref).abs().max().item()
        assert err < 1.5e-2, (j, err)
        moved = (out.float() - base.float()).abs().amax(dim=1)
        assert (moved[first:] > 3e-2).all(), (j, moved)
        assert torch.equal(out[:first], base[:first]), f"key {j}: a row that cannot see it moved"


# ------------------------------------------------------------------ 2. the block against the existing pair
@pytest.fixture(scope="module")
def engine2k():
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=CTX))
    W = O.make_weights(cfg, seed=1)
    return cfg, W, make_hip_model(cfg, W, torch.bfloat16)


@pytest.mark.parametrize("T,P", [(5, 33), (40, 600), (64, 1900), (65, 600), (200, 1000)])
def test_llama_extend_vs_prefill(engine2k, T, P):
    """vcla_llama_extend and vcla_llama_prefill(pos0 = P) on equal cache contents: logits within 0.2 max / 0.04 mean and the K / V rows both
    write within 0.15, the bounds two bf16 forms of one model are held to at these widths (tests/test_gpu_engine.py)"""
    from visualcla.modeling_visualcla import VclaCache
    cfg, W, m = engine2k
    g = torch.Generator().manual_seed(T * 7 + P)
    ids = torch.randint(3, cfg.text.vocab_size - 8, (1, P + T), generator=g).to(DEV)
    emb, _ = m._embed(ids, None, None)
    base = m._new_cache(1, CTX)
    base.kv.zero_()
    m._prefill(emb[:, :P].contiguous(), base, None, all_logits=False)       # a real conversation's rows [0, P)
    a, b = VclaCache(base.kv.clone(), P, CTX), VclaCache(base.kv.clone(), P, CTX)
    la = m._prefill(emb[:, P:].contiguous(), a, None, all_logits=False).clone()
    lb = m._extend(emb[:, P:].contiguous(), b).clone()
    torch.cuda.synchronize()
    dl = (la - lb).abs()
    dkv = (a.kv[..., P:P + T, :].float() - b.kv[..., P:P + T, :].float()).abs().max().item()
    print(f"[llama_extend] T {T} P {P}: logits max {dl.max().item():.3e} mean {dl.mean().item():.3e}, rows max {dkv:.3e}")
    assert torch.isfinite(lb).all()
    assert dl.max().item() <= 0.2 and dl.mean().item() <= 0.04, (T, P, dl.max().item(), dl.mean().item())
    assert dkv <= 0.15, (T, P, dkv)
    assert torch.equal(a.kv[..., :P, :], b.kv[..., :P, :]) and torch.equal(b.kv[..., P + T:, :], base.kv[..., P + T:, :])
    assert (b.kv[..., P:P + T, :].float().abs().amax(dim=-1) > 0).all()      # every (layer, k / v, head) row of the block was appended


# ------------------------------------------------------------------ 3. fp32: the oracle's ids over three turns
def _common_prefix(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def _three_turns(cfg, W):
    """prompts of the three turns and the oracle's greedy ids for each; turn 3 diverges inside the rows turn 2 generated"""
    Q = cfg.resampler.num_query_tokens
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    px, prompt, _ = O.make_inputs(cfg, 1, 40 + Q, seed_ids=701)
    g = torch.Generator().manual_seed(702)
    prompts, wants, margin = [], [], float("inf")
    for k in range(3):
        toks, logits = O.visualcla_generate(prompt, px, torch.ones_like(prompt), W, cfg, max_new_tokens=12, return_logits=True)
        for lg in logits:
            top2 = lg[0].topk(2).values
            margin = min(margin, float(top2[0] - top2[1]))
        prompts.append(prompt)
        wants.append(toks)
        kept = toks[:, :12] if k == 0 else toks[:, :6]
        prompt = torch.cat([prompt, kept, torch.randint(3, hi, (1, 10 - k), generator=g)], dim=1)
    return px, prompts, wants, margin


@pytest.mark.parametrize("which", ["tiny", "small"])
def test_three_turns_equal_the_oracle_fp32(which):
    cfg = O.cfg_tiny() if which == "tiny" else O.cfg_small()
    W = O.make_weights(cfg, seed=0)
    px, prompts, wants, margin = _three_turns(cfg, W)
    print(f"[session] {which}: prompt lengths {[p.shape[1] for p in prompts]}, smallest top-2 margin {margin:.3e}")
    assert [p.shape[1] for p in prompts] == ([48, 70, 85] if which == "tiny" else [56, 78, 93])
    assert margin >= 1e-4, f"margin {margin:.2e} -- pick other seeds, equality of ids is not decidable here"
    m = make_hip_model(cfg, W, torch.float32)
    s = m.new_session()
    held = []
    for k, (prompt, want) in enumerate(zip(prompts, wants)):
        kw = dict(input_ids=prompt.cuda(), pixel_values=px.cuda(), max_new_tokens=12, do_sample=False, eos_token_id=None)
        plain = m.generate(**kw).cpu()
        got = m.generate(session=s, **kw).cpu()
        st = dict(m.last_session_stats)
        assert torch.equal(plain, want) and torch.equal(got, want), (k, got.tolist(), want.tolist())
        T = prompt.shape[1]
        exp = min(_common_prefix(prompt[0].tolist(), held), T - 1)
        assert st == {"reused": exp, "prefilled": T - exp, "vision_skipped": k > 0}, (k, st, exp)
        if k == 1:
            assert exp == prompts[0].shape[1] + 11
        if k == 2:
            assert exp >= prompts[1].shape[1] + 6
        held = prompt[0].tolist() + got[0].tolist()[:-1]
        assert s.ids == held and s.length == len(held)


# ------------------------------------------------------------------ 4. bf16 at the engine widths
def _steps_vs_oracle(m, cfg, W, ids, session):
    """first-token logits and four teacher-forced decode steps of generate() against the fp32 oracle on the full prompt:
    [(max, mean, hip argmax, oracle argmax, oracle margin)]"""
    from transformers import LogitsProcessorList
    seen = []

    def grab(ids_, scores):
        seen.append(scores.detach().float().cpu().clone())
        return scores
    kw = {} if session is None else {"session": session}
    toks = m.generate(input_ids=ids.cuda(), max_new_tokens=5, do_sample=False, eos_token_id=None, logits_processor=LogitsProcessorList([grab]), **kw).cpu()
    T = ids.shape[1]
    with torch.no_grad():
        cache = [None] * cfg.text.num_hidden_layers
        h = O.llama_forward(O.embed_and_splice(ids, None, W, cfg), W, cfg.text, torch.ones(1, T, dtype=torch.int64), cache, 0)
        refs = [O.lm_head(h[:, -1:], W)[:, 0]]
        for i in range(4):
            e = W["text_model.model.embed_tokens.weight"][toks[:, i]][:, None, :]
            h = O.llama_forward(e, W, cfg.text, torch.ones(1, T + i + 1, dtype=torch.int64), cache, T + i)
            refs.append(O.lm_head(h, W)[:, 0])
    out = []
    for i in range(5):
        dl = (seen[i] - refs[i]).abs()
        top2 = refs[i].topk(2, dim=-1).values[0]
        out.append((dl.max().item(), dl.mean().item(), int(seen[i].argmax()), int(refs[i].argmax()), float(top2[0] - top2[1])))
    return out


def test_session_turn_bf16_engine_widths():
    """two turns at the LLaMA-7B widths (T1 = 33, 24 generated, 20 new ids): the turn-2 logits on the session's rows against the fp32 oracle on the
    full prompt within the bounds test_engine_steps_match_the_oracle holds this config to, and no further from it than the same turn re-prefilled"""
    cfg = cfg_engine_small()
    W = O.make_weights(cfg, seed=1)
    m = make_hip_model(cfg, W, torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    ids1 = torch.randint(3, cfg.text.vocab_size - 8, (1, 33), generator=g)
    s = m.new_session()
    t1 = m.generate(input_ids=ids1.cuda(), max_new_tokens=24, do_sample=False, eos_token_id=None, session=s).cpu()
    ids2 = torch.cat([ids1, t1, torch.randint(3, cfg.text.vocab_size - 8, (1, 20), generator=g)], dim=1)
    with_s = _steps_vs_oracle(m, cfg, W, ids2, s)
    assert m.last_session_stats == {"reused": 33 + 23, "prefilled": 21, "vision_skipped": False}
    without = _steps_vs_oracle(m, cfg, W, ids2, None)
    for i, ((mx, mean, a_hip, a_ref, margin), (mx0, mean0, *_)) in enumerate(zip(with_s, without)):
        print(f"[session bf16] step {i}: session max {mx:.3e} mean {mean:.3e}; re-prefilled max {mx0:.3e} mean {mean0:.3e}; oracle margin {margin:.3e}")
    for i, ((mx, mean, a_hip, a_ref, margin), (mx0, mean0, *_)) in enumerate(zip(with_s, without)):
        assert mx < 0.12 and mean < 0.022, (i, mx, mean)
        assert margin < 0.24 or a_hip == a_ref, (i, a_hip, a_ref, margin)
        assert mean <= 1.25 * mean0 + 1e-3, (i, mean, mean0)


# ------------------------------------------------------------------ 5. an empty session is the existing path
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_empty_session_is_the_existing_path(dt):
    cfg = O.cfg_small()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), dt)
    px, ids, _ = O.make_inputs(cfg, 1, 64, seed_ids=31)
    for kw in (dict(do_sample=False), dict(do_sample=True, top_k=30, top_p=0.9, temperature=0.8, repetition_penalty=1.1)):
        kw.update(input_ids=ids.cuda(), pixel_values=px.cuda(), max_new_tokens=20, eos_token_id=None)
        torch.manual_seed(11)
        plain = m.generate(**kw).cpu()
        torch.manual_seed(11)
        got = m.generate(session=m.new_session(), **kw).cpu()
        assert m.last_session_stats == {"reused": 0, "prefilled": ids.shape[1], "vision_skipped": False}
        assert torch.equal(plain, got), (dt, kw["do_sample"], plain.tolist(), got.tolist())


# ------------------------------------------------------------------ 6. image change, reset, two sessions, sampling, refusals
def test_session_image_change_reset_and_two_sessions():
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    g = torch.Generator().manual_seed(5)
    px, ids, _ = O.make_inputs(cfg, 1, 44, seed_ids=51)
    px2 = torch.randn(px.shape, generator=g)
    kw = dict(max_new_tokens=8, do_sample=False, eos_token_id=None)

    def turn2(first, toks):
        return torch.cat([first, toks, torch.randint(3, hi, (1, 7), generator=g)], dim=1)
    s = m.new_session()
    t = cfg.text
    assert s.length == 0 and s.capacity == t.max_position_embeddings and s.nbytes == t.num_hidden_layers * 2 * t.hidden_size * s.capacity * 4
    t1 = m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=s, **kw).cpu()
    ids2 = turn2(ids, t1)
    # another image under the same ids: nothing is reused, the vision stack runs
    got = m.generate(input_ids=ids2.cuda(), pixel_values=px2.cuda(), session=s, **kw).cpu()
    assert m.last_session_stats == {"reused": 0, "prefilled": ids2.shape[1], "vision_skipped": False}
    assert torch.equal(got, m.generate(input_ids=ids2.cuda(), pixel_values=px2.cuda(), **kw).cpu())
    # ... and the session now belongs to that image
    ids3 = turn2(ids2, got)
    got3 = m.generate(input_ids=ids3.cuda(), pixel_values=px2.clone().cuda(), session=s, **kw).cpu()
    assert m.last_session_stats["reused"] == ids2.shape[1] + 7 and m.last_session_stats["vision_skipped"]
    assert torch.equal(got3, m.generate(input_ids=ids3.cuda(), pixel_values=px2.cuda(), **kw).cpu())
    s.reset()
    assert s.length == 0 and s.ids == []
    m.generate(input_ids=ids3.cuda(), pixel_values=px2.cuda(), session=s, **kw)
    assert m.last_session_stats["reused"] == 0
    # two sessions used alternately return what each returns alone
    _, idsb, _ = O.make_inputs(cfg, 1, 40, seed_ids=52)
    alone = {}
    for name, first in (("a", ids), ("b", idsb)):
        sa = m.new_session()
        x1 = m.generate(input_ids=first.cuda(), pixel_values=px.cuda(), session=sa, **kw).cpu()
        second = turn2(first, x1)
        alone[name] = (x1, second, m.generate(input_ids=second.cuda(), pixel_values=px.cuda(), session=sa, **kw).cpu())
    sa, sb = m.new_session(), m.new_session()
    a1 = m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=sa, **kw).cpu()
    b1 = m.generate(input_ids=idsb.cuda(), pixel_values=px.cuda(), session=sb, **kw).cpu()
    a2 = m.generate(input_ids=alone["a"][1].cuda(), pixel_values=px.cuda(), session=sa, **kw).cpu()
    ra = m.last_session_stats["reused"]
    b2 = m.generate(input_ids=alone["b"][1].cuda(), pixel_values=px.cuda(), session=sb, **kw).cpu()
    rb = m.last_session_stats["reused"]
    assert torch.equal(a1, alone["a"][0]) and torch.equal(a2, alone["a"][2]) and torch.equal(b1, alone["b"][0]) and torch.equal(b2, alone["b"][2])
    assert ra == ids.shape[1] + 7 and rb == idsb.shape[1] + 7
    # a model rebuilt since the rows were written (here: another dtype) empties its sessions
    m.half()
    m.generate(input_ids=alone["a"][1].cuda(), pixel_values=px.cuda(), session=sa, **kw)
    assert m.last_session_stats["reused"] == 0 and sa.kv.dtype == torch.bfloat16 and sa.nbytes == s.nbytes // 2


def test_session_sampling_draws_what_generate_draws_fp32():
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    px, ids, _ = O.make_inputs(cfg, 1, 44, seed_ids=61)
    kw = dict(max_new_tokens=10, do_sample=True, top_k=12, top_p=0.95, temperature=0.9, eos_token_id=None)
    s = m.new_session()
    torch.manual_seed(3)
    t1 = m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=s, **kw).cpu()
    ids2 = torch.cat([ids, t1, torch.randint(3, hi, (1, 9), generator=torch.Generator().manual_seed(62))], dim=1)
    torch.manual_seed(4)
    want = m.generate(input_ids=ids2.cuda(), pixel_values=px.cuda(), **kw).cpu()
    torch.manual_seed(4)
    got = m.generate(input_ids=ids2.cuda(), pixel_values=px.cuda(), session=s, **kw).cpu()
    assert m.last_session_stats["reused"] == ids.shape[1] + 9
    assert torch.equal(got, want)


def test_session_refusals_on_the_device():
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    px, ids, _ = O.make_inputs(cfg, 1, 44, seed_ids=71)
    s = m.new_session()
    mask = torch.ones_like(ids)
    mask[0, 0] = 0
    with pytest.raises(ValueError, match="attention_mask"):
        m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), attention_mask=mask.cuda(), session=s, max_new_tokens=3)
    with pytest.raises(ValueError, match="batch size 2"):
        m.generate(input_ids=torch.cat([ids, ids]).cuda(), pixel_values=torch.cat([px, px]).cuda(), session=s, max_new_tokens=3)
    with pytest.raises(ValueError, match="num_beams=2, num_return_sequences=2"):
        m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=s, max_new_tokens=3, num_beams=2, num_return_sequences=2)
    with pytest.raises(ValueError, match="session=.*prompt_lookup_num_tokens=3"):
        m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=s, max_new_tokens=3, do_sample=False, prompt_lookup_num_tokens=3)
    other = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    with pytest.raises(ValueError, match="new_session"):
        other.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=s, max_new_tokens=3)
    small = m.new_session(max_tokens=ids.shape[1])
    with pytest.raises(ValueError, match="capacity"):
        m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), session=small, max_new_tokens=3)
    # an all-ones mask is no mask; a refused call leaves the session usable
    got = m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), attention_mask=torch.ones_like(ids).cuda(), session=s, max_new_tokens=3, do_sample=False)
    assert torch.equal(got.cpu(), m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), max_new_tokens=3, do_sample=False).cpu())


# ------------------------------------------------------------------ 7. neighbours keep working
def test_neighbours_unchanged_by_sessions():
    from tests.test_gpu_inflight import _as_dicts, _requests
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    reqs = _requests(cfg)
    ids1 = reqs[11][0].cuda()
    px, ids, _ = O.make_inputs(cfg, 1, 48, seed_ids=9)

    def neighbours():
        a = m.generate(input_ids=ids1, max_new_tokens=24, do_sample=False, eos_token_id=None).cpu()
        b = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None)
        c = m.generate(input_ids=ids1, max_new_tokens=24, do_sample=False, eos_token_id=None, prompt_lookup_num_tokens=3).cpu()
        return a, [x.cpu() for x in b], c
    before = neighbours()
    s = m.new_session()
    t1 = m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), max_new_tokens=10, do_sample=False, eos_token_id=None, session=s).cpu()
    ids2 = torch.cat([ids, t1, ids1[:, 1:8].cpu()], dim=1)
    m.generate(input_ids=ids2.cuda(), pixel_values=px.cuda(), max_new_tokens=10, do_sample=False, eos_token_id=None, session=s)
    assert m.last_session_stats["reused"] == ids.shape[1] + 9
    after = neighbours()
    assert torch.equal(before[0], after[0]) and torch.equal(before[2], after[2]) and torch.equal(before[0], before[2])
    assert all(torch.equal(x, y) for x, y in zip(before[1], after[1]))


# ------------------------------------------------------------------ 8. chat(session=) on the real tokenizer
from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_with_a_session_equals_chat(loaded, capsys):  # noqa: F811
    """two turns through chat(): the second prompt holds the first response RE-TOKENISED from its text; the common-prefix rule absorbs whatever
    that changes, so responses and histories are those of chat() without a session and nearly all of turn 1 is reused"""
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    gc = GenerationConfig(max_new_tokens=9, do_sample=False)
    img = _image()
    texts = ["what is this?", "describe the image again"]
    want, hist = [], []
    for text in texts:
        want.append(visualcla.chat(model, img, text, history=hist, generation_config=gc)[0])
    s = model.new_session()
    got, hist_s, stats = [], [], []
    for text in texts:
        got.append(visualcla.chat(model, img, text, history=hist_s, generation_config=gc, session=s)[0])
        stats.append(dict(model.last_session_stats))
    capsys.readouterr()
    assert got == want and hist_s == hist and len(hist_s) == 4
    T1 = stats[0]["prefilled"]
    assert stats[0]["reused"] == 0 and not stats[0]["vision_skipped"]
    print(f"[session chat] turn 1 prompt {T1} tokens; turn 2 {stats[1]}")
    assert stats[1]["reused"] >= T1 - 2 and stats[1]["vision_skipped"], stats

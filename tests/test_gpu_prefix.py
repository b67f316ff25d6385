"""Prefix sharing on the MI355X: vcla_attn_extend_rows against arithmetic and against vcla_rope_kv_append,
vcla_llama_extend_rows against vcla_llama_extend per sequence, generate_many(share_prefix=True) against the CPU oracle, against
generate_many() without sharing and against the plan's row accounting."""
import dataclasses
import random

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


def _extend_rows(qkv, kv, cos, sin, table, H, d, frag=0):
    """-> (out [M, H d] bf16, scratch bytes); kv [2, B_slots, H, CTX, d] is updated in place; table = [(slot, pos, rows)]"""
    L = _lib()
    lib = L.load()
    seqs, M = L.extend_seqs(table)
    nb = lib.vcla_attn_extend_rows_scratch_bytes(seqs, len(table), H, d)
    assert 0 < nb <= lib.vcla_attn_extend_rows_scratch_bound(M, len(table), H, d), (nb, M, len(table))
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    rows = (M + 15) // 16 * 16 if frag else M
    out = torch.zeros(rows * H * d, dtype=torch.bfloat16, device=DEV)
    L.check(lib.vcla_attn_extend_rows(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), seqs, len(table), M,
                                      kv.shape[1], H, d, CTX, d ** -0.5, L.VCLA_BF16, frag, 0, scratch.data_ptr(), scratch.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    if frag:
        return L.from_frag(out.view((H * d) // 32, rows // 16, 64, 8), M), nb
    return out.view(M, H * d), nb


def _attention_ref(qkv, kv_slot, cos, sin, R, H, d, p):
    """fp32 attention of one block from the same bf16 inputs: rotated q against ITS slot's cache as it stands after the append"""
    q = _rope_ref(qkv[:, :H * d].float().view(R, H, d), cos[p:p + R], sin[p:p + R])
    K, V = kv_slot[0, :, :p + R].float(), kv_slot[1, :, :p + R].float()
    s = torch.einsum("rhd,hjd->rhj", q, K) * d ** -0.5
    vis = torch.arange(p + R, device=DEV)[None, :] <= (p + torch.arange(R, device=DEV))[:, None]
    s = s.masked_fill(~vis[:, None, :], float("-inf"))
    return torch.einsum("rhj,hjd->rhd", torch.softmax(s, dim=-1), V).reshape(R, H * d)


def _check_table(table, B_slots, H, d, g, kv0, cos, sin, tag):
    """the three claims of test_attn_extend_vs_arithmetic per block, plus: nothing outside the blocks moved.  -> (worst error, scratch bytes)"""
    L = _lib()
    lib = L.load()
    M = sum(r for _, _, r in table)
    qkv = torch.randn(M, 3 * H * d, generator=g).to(torch.bfloat16).to(DEV)
    kv = kv0.clone()
    out, nb = _extend_rows(qkv, kv, cos, sin, table, H, d)
    touched = torch.zeros(B_slots, CTX, dtype=torch.bool, device=DEV)
    worst, m0 = 0.0, 0
    for slot, p, R in table:
        blk = qkv[m0:m0 + R].contiguous()
        kv_ref = kv0[:, slot].clone()
        L.check(lib.vcla_rope_kv_append(blk.clone().data_ptr(), kv_ref[0].data_ptr(), kv_ref[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, R, H, d, CTX, p,
                                        None, L.VCLA_BF16, L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(kv[:, slot, :, p:p + R], kv_ref[:, :, p:p + R]), f"{tag} slot {slot} R {R} p {p}: appended rows differ from vcla_rope_kv_append's"
        touched[slot, p:p + R] = True
        err = (out[m0:m0 + R].float() - _attention_ref(blk, kv[:, slot], cos, sin, R, H, d, p)).abs().max().item()
        worst = max(worst, err)
        assert err < 1.5e-2, f"{tag} slot {slot} R {R} p {p}: max |err| {err}"
        m0 += R
    same = (kv == kv0).all(dim=-1).all(dim=0).all(dim=1)               # [B_slots, CTX]: the row is unchanged in K and V of every head
    assert bool(same[~touched].all()), f"{tag}: a cache row outside the appended ranges changed"
    if M <= 64:
        kv_f = kv0.clone()
        out_f, _ = _extend_rows(qkv, kv_f, cos, sin, table, H, d, frag=1)
        assert torch.equal(out_f, out) and torch.equal(kv_f, kv), f"{tag}: the fragment-major output differs"
    return worst, nb


def _mixed_table(rng, n, B_slots, rows, poss):
    slots = list(range(B_slots))
    rng.shuffle(slots)
    table = []
    for i in range(n):
        R = rows[i % len(rows)]
        p = poss[(i * 3 + n) % len(poss)]
        if p + R > CTX:
            p = CTX - R
        table.append((slots[i], p, R))
    return table


@pytest.mark.parametrize("n,H", [(1, 32), (5, 32), (17, 3), (64, 8)])
def test_attn_extend_rows_vs_arithmetic(n, H):
    """mixed tables in shuffled slots of a larger cache: every block within atol 1.5e-2 of fp32 attention over ITS slot (the bound of
    test_attn_extend_vs_arithmetic), its appended rows bitwise vcla_rope_kv_append's, every other cache row of every slot untouched, the
    fragment-major output (M <= 64) the same bits"""
    d = 128
    B_slots = n + 3
    rng = random.Random(100 + n)
    g = torch.Generator().manual_seed(100 + n)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(CTX, d, 10000.0))
    kv0 = torch.randn(2, B_slots, H, CTX, d, generator=g).to(torch.bfloat16).to(DEV)
    tables = [
        _mixed_table(rng, n, B_slots, [38, 1, 256, 17, 64, 100, 5, 128, 65, 33], [90, 0, 1900, 63, 0, 511, 1, 1000, 200, 512]),
        _mixed_table(rng, n, B_slots, [128], [0]),                                     # nothing to share: the common case
        _mixed_table(rng, n, B_slots, [38], [90]),
        _mixed_table(rng, n, B_slots, [1, 2, 3, 4, 7] if n > 5 else [1, 7, 16, 17, 20], [0, 700, 1900, 64, 1]),   # M <= 64: both layouts
    ]
    if n == 1:
        tables += [[(2, 1900, 38)], [(0, 1792, 256)], [(3, 0, 1)], [(1, 1000, 64)]]    # one long block: the splits and the merge
    worst, split_cases, frag_cases = 0.0, 0, 0
    for k, table in enumerate(tables):
        if sum(r for _, _, r in table) > 64 and n == 64 and k == 3:
            table = [(s, p, 1) for s, p, _ in table]
        assert any(p == 0 for _, p, _ in table) or k == 2 or n == 1
        L = _lib()
        seqs, M = L.extend_seqs(table)
        lists_only = L.load().vcla_attn_extend_rows_scratch_bytes(seqs, len(table), 1 << 20, d)     # H so large that nothing is split: the lists alone
        err, nb = _check_table(table, B_slots, H, d, g, kv0, cos, sin, f"n {n} table {k}")
        split_cases += nb > (lists_only + 4096)
        frag_cases += M <= 64
        worst = max(worst, err)
        print(f"[attn_extend_rows] n {n} H {H} table {k}: M {M} scratch {nb} B, max |err| {err:.3e}")
    print(f"[attn_extend_rows] n {n} H {H}: worst max |err| {worst:.3e}; {split_cases} tables with split work items, {frag_cases} with both layouts")
    assert frag_cases >= 1
    if n in (1, 5, 17):
        assert split_cases >= 1            # the merge launch is not covered by accident


def test_attn_extend_rows_head_dim_64():
    d, H, B_slots = 64, 5, 9
    rng = random.Random(64)
    g = torch.Generator().manual_seed(64)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(CTX, d, 10000.0))
    kv0 = torch.randn(2, B_slots, H, CTX, d, generator=g).to(torch.bfloat16).to(DEV)
    for k, table in enumerate([_mixed_table(rng, 6, B_slots, [1, 7, 33, 64, 100, 256], [0, 30, 63, 700, 1, 1500]),
                               _mixed_table(rng, 5, B_slots, [7, 16, 1, 20, 17], [0, 1900, 64, 0, 511]),
                               [(4, 1792, 256)], [(8, 1900, 40)]]):
        err, nb = _check_table(table, B_slots, H, d, g, kv0, cos, sin, f"d64 table {k}")
        print(f"[attn_extend_rows d64] table {k}: scratch {nb} B, max |err| {err:.3e}")


def test_attn_extend_rows_refuses_bad_tables():
    """a slot named twice, a block past ctx_max, blocks not packed back to back, too small a scratch: refused by name, nothing written"""
    L = _lib()
    lib = L.load()
    H, d = 2, 64
    kv = torch.zeros(2, 3, H, CTX, d, dtype=torch.bfloat16, device=DEV)
    qkv = torch.ones(8, 3 * H * d, dtype=torch.bfloat16, device=DEV)
    tab = torch.zeros(CTX, d // 2, device=DEV)
    out = torch.zeros(8, H * d, dtype=torch.bfloat16, device=DEV)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)

    def call(table, M=8, n_scratch=1 << 20, row0=None):
        seqs, _ = L.extend_seqs(table)
        if row0 is not None:
            seqs[1].row0 = row0
        L.check(lib.vcla_attn_extend_rows(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), tab.data_ptr(), tab.data_ptr(), out.data_ptr(), seqs, len(table), M, 3, H,
                                          d, CTX, 1.0, L.VCLA_BF16, 0, 0, scratch.data_ptr(), n_scratch, L.stream_ptr()))
    for kw, msg in ((dict(table=[(1, 0, 4), (1, 9, 4)]), "named twice"), (dict(table=[(0, CTX - 3, 4), (1, 0, 4)]), "ctx_max"),
                    (dict(table=[(0, 0, 4), (1, 0, 4)], row0=5), "expected 4"), (dict(table=[(0, 0, 4), (3, 0, 4)]), "slot 3"),
                    (dict(table=[(0, 0, 4), (1, 0, 3)]), "M=8"), (dict(table=[(0, 0, 4), (1, 0, 4)], n_scratch=16), "scratch")):
        with pytest.raises((ValueError, L.VclaError), match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert not kv.any() and not out.any()


def test_attn_extend_rows_planted_key():
    """test_attn_extend_planted_key with neighbours: one key made to matter (value row 100, score 0), planted at the tile, split and p seams of
    block A's own slot -- the rows of A that may see it move far outside the bound, rows that may not and BOTH other blocks keep their bits --
    and in the neighbouring slots at the same positions: A keeps its bits (a block that read another sequence's cache would not)"""
    H, d, B_slots = 3, 128, 5
    R, p = 40, 700
    table = [(3, 300, 33), (2, p, R), (1, p, R), (4, 0, 20)]           # block A = (slot 2, p, R): a neighbour at the same p in slot 1, another in slot 3
    m0 = 33
    g = torch.Generator().manual_seed(77)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(CTX, d, 10000.0))
    kv0 = torch.randn(2, B_slots, H, CTX, d, generator=g).to(torch.bfloat16).to(DEV)
    M = sum(r for _, _, r in table)
    qkv0 = torch.randn(M, 3 * H * d, generator=g).to(torch.bfloat16).to(DEV)
    base, _ = _extend_rows(qkv0, kv0.clone(), cos, sin, table, H, d)
    per = 128                                                           # a split seam whatever the rule picks lies on a tile seam: cover several
    a_rows = slice(m0, m0 + R)
    for j in (0, 63, 64, per - 1, per, 2 * per - 1, 2 * per, 383, 384, p - 1, p, p + 20, p + R - 1):
        kv, qkv = kv0.clone(), qkv0.clone()
        if j < p:
            kv[0, 2, :, j] = 0
            kv[1, 2, :, j] = 100.0
        else:
            qkv.view(M, 3, H, d)[m0 + j - p, 1] = 0
            qkv.view(M, 3, H, d)[m0 + j - p, 2] = 100.0
        out, _ = _extend_rows(qkv, kv, cos, sin, table, H, d)
        ref = _attention_ref(qkv[a_rows].contiguous(), kv[:, 2], cos, sin, R, H, d, p)
        first = max(0, j - p)
        err = (out[a_rows].float() - ref).abs().max().item()
        assert err < 1.5e-2, (j, err)
        moved = (out[a_rows].float() - base[a_rows].float()).abs().amax(dim=1)
        assert (moved[first:] > 3e-2).all(), (j, moved)
        assert torch.equal(out[m0:m0 + first], base[m0:m0 + first]), f"key {j}: a row of the block that cannot see it moved"
        assert torch.equal(out[:m0], base[:m0]) and torch.equal(out[m0 + R:], base[m0 + R:]), f"key {j}: another block moved"
    # the same key in a neighbouring slot (one in the table at the same p, one not in the table): block A must not see it
    for slot in (1, 0):
        for j in (0, 64, p - 1, p, p + R - 1):
            kv = kv0.clone()
            kv[0, slot, :, j] = 0
            kv[1, slot, :, j] = 100.0
            out, _ = _extend_rows(qkv0, kv, cos, sin, table, H, d)
            assert torch.equal(out[a_rows], base[a_rows]), f"slot {slot} key {j}: block A read a neighbour's cache"
            if slot == 1 and j < p:
                nb_rows = slice(m0 + R, m0 + 2 * R)
                assert ((out[nb_rows].float() - base[nb_rows].float()).abs().amax(dim=1) > 3e-2).all()        # ... while its owner does
            else:
                assert torch.equal(out, base)                          # a row the owner overwrites (j >= p) or a slot nobody reads


# ------------------------------------------------------------------ 2. the pass against vcla_llama_extend per sequence
@pytest.fixture(scope="module")
def engine2k():
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=CTX))
    W = O.make_weights(cfg, seed=1)
    return cfg, W, make_hip_model(cfg, W, torch.bfloat16)


@pytest.mark.parametrize("name,table", [("stream", [(2, 33, 5), (0, 0, 20), (3, 600, 30)]),
                                        ("stream1", [(1, 90, 38)]),
                                        ("stream_m1", [(3, 63, 1)]),             # M = 1 (a duplicate prompt capped at T - 1): llama_layer's GEMV branch
                                        ("tile", [(1, 600, 40), (0, 0, 128), (4, 1000, 65), (2, 90, 38)]),
                                        ("tile_p0", [(3, 0, 128), (1, 0, 100), (0, 0, 7)])])
def test_llama_extend_rows_vs_extend_per_sequence(engine2k, name, table):
    """vcla_llama_extend_rows and vcla_llama_extend once per sequence on equal cache contents: logits within 0.2 max / 0.04 mean, appended rows
    within 0.15 (the bounds of test_llama_extend_vs_prefill), for tables on the streaming route (M <= 64) and on the tile route; everything
    outside the blocks bitwise untouched"""
    from visualcla.modeling_visualcla import VclaCache
    cfg, W, m = engine2k
    B_slots = 5
    g = torch.Generator().manual_seed(sum(p + r for _, p, r in table))
    M = sum(r for _, _, r in table)
    assert (M <= 64) == name.startswith("stream")
    t = cfg.text
    slots_kv = (torch.randn(t.num_hidden_layers, 2, B_slots, t.num_attention_heads, CTX, t.hidden_size // t.num_attention_heads, generator=g) * 0.1) \
        .to(torch.bfloat16).to(DEV)
    embs, refs = [], []
    for slot, P, T in table:
        ids = torch.randint(3, t.vocab_size - 8, (1, P + T), generator=g).to(DEV)
        emb, _ = m._embed(ids, None, None)
        own = m._new_cache(1, CTX)
        own.kv.copy_(slots_kv[:, :, slot:slot + 1])
        if P:
            m._prefill(emb[:, :P].contiguous(), own, None, all_logits=False)          # a real prompt's rows [0, P)
            slots_kv[:, :, slot, :, :P] = own.kv[:, :, 0, :, :P]
        c = VclaCache(own.kv, P, CTX)
        lg = (m._extend(emb[:, P:].contiguous(), c) if T > 1 else m._prefill(emb[:, P:].contiguous(), c, None, all_logits=False)).clone()
        refs.append((lg, own.kv[:, :, 0].clone()))
        embs.append(emb[0, P:])
    before = slots_kv.clone()
    logits = m._extend_rows(torch.cat(embs), table, slots_kv)
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
    touched = torch.zeros(B_slots, CTX, dtype=torch.bool, device=DEV)
    for i, ((slot, P, T), (lg, kv_ref)) in enumerate(zip(table, refs)):
        dl = (logits[i] - lg[0]).abs()
        dkv = (slots_kv[:, :, slot, :, P:P + T].float() - kv_ref[:, :, :, P:P + T].float()).abs().max().item()
        print(f"[llama_extend_rows] {name} block {i} (slot {slot} P {P} T {T}): logits max {dl.max().item():.3e} mean {dl.mean().item():.3e}, rows max {dkv:.3e}")
        assert dl.max().item() <= 0.2 and dl.mean().item() <= 0.04, (name, i, dl.max().item(), dl.mean().item())
        assert dkv <= 0.15, (name, i, dkv)
        assert (slots_kv[:, :, slot, :, P:P + T].float().abs().amax(dim=-1) > 0).all()
        touched[slot, P:P + T] = True
    same = (slots_kv == before).all(dim=-1).all(dim=3).all(dim=0).all(dim=0)          # [B_slots, CTX]
    assert bool(same[~touched].all()), f"{name}: a cache row outside the blocks changed"


def test_llama_extend_rows_fp32_route_and_refusals():
    """fp32 takes the block-by-block route: logits and rows equal vcla_llama_prefill(B = 1, pos0) on the slot to fp32 rounding; the e4m3 cache is
    refused by name"""
    from visualcla.modeling_visualcla import VclaCache
    cfg = O.cfg_small()
    W = O.make_weights(cfg, seed=0)
    m = make_hip_model(cfg, W, torch.float32)
    t = cfg.text
    ctx, B_slots = 128, 4
    g = torch.Generator().manual_seed(3)
    table = [(2, 20, 9), (0, 0, 31), (3, 50, 1)]
    kv = torch.zeros(t.num_hidden_layers, 2, B_slots, t.num_attention_heads, ctx, t.hidden_size // t.num_attention_heads, device=DEV)
    embs, refs = [], []
    for slot, P, T in table:
        ids = torch.randint(3, 200, (1, P + T), generator=g).to(DEV)
        emb, _ = m._embed(ids, None, None)
        own = m._new_cache(1, ctx)
        own.kv.zero_()
        if P:
            m._prefill(emb[:, :P].contiguous(), own, None, all_logits=False)
            kv[:, :, slot, :, :P] = own.kv[:, :, 0, :, :P]
        lg = m._prefill(emb[:, P:].contiguous(), VclaCache(own.kv, P, ctx), None, all_logits=False).clone()
        refs.append((lg, own.kv[:, :, 0].clone()))
        embs.append(emb[0, P:])
    logits = m._extend_rows(torch.cat(embs), table, kv)
    for i, ((slot, P, T), (lg, kv_ref)) in enumerate(zip(table, refs)):
        assert (logits[i] - lg[0]).abs().max().item() < 1e-4, i
        assert (kv[:, :, slot, :, :P + T] - kv_ref[:, :, :, :P + T]).abs().max().item() < 1e-5, i
    assert not kv[:, :, 1].any()
    ecfg = cfg_engine_small()
    m16 = make_hip_model(ecfg, O.make_weights(ecfg, seed=3), torch.bfloat16)
    m16.enable_fp8_decode(True, prefill=False, kv_cache=True)
    et = ecfg.text
    kv8 = torch.zeros(et.num_hidden_layers, 2, B_slots, et.num_attention_heads, ctx, et.hidden_size // et.num_attention_heads, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="e4m3"):
        m16._extend_rows(torch.ones(sum(r for _, _, r in table), et.hidden_size, dtype=torch.bfloat16, device=DEV), table, kv8)
    assert not kv8.any()


# ------------------------------------------------------------------ 3. end to end, fp32: the oracle's ids, the ids without sharing, the plan's rows
BUDGETS = [12, 3, 20, 7, 1, 16, 9, 24, 5, 14, 10, 18, 6, 11]
BASE = 901          # the smallest top-2 margin over all steps of this queue is asserted below; base 900 fails that assertion on the tiny config


def _queue(cfg, base=BASE):
    """14 requests: a head of BOS + 20 ids common to ALL; three images x three questions (tails of 6..22 ids), arrival interleaved by image;
    request 9 = request 0 + 7 more ids (request 0 is a strict prefix of it); two text-only requests with a common 24-id text behind the head;
    request 12: the ids of request 1 with another image; request 13: nothing in common with anyone (its own head)."""
    Q = cfg.resampler.num_query_tokens
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    g = torch.Generator().manual_seed(base)
    r = lambda n: torch.randint(3, hi, (n,), generator=g)          # noqa: E731
    head = torch.cat([torch.tensor([1]), r(20)])
    slot = torch.tensor([cfg.img_start_token_id] + [cfg.img_token_id] * Q + [cfg.img_end_token_id])
    px = [O.make_inputs(cfg, 1, Q + 3 + 1 + 4, seed_pixels=base + 50 + k)[0] for k in range(4)]
    reqs = [None] * 14
    for q in range(3):
        for k in range(3):
            i = q * 3 + k
            reqs[i] = (torch.cat([head, slot, r(6 + 2 * i)])[None], px[k])
    reqs[9] = (torch.cat([reqs[0][0][0], r(7)])[None], px[0])
    text = r(24)
    reqs[10] = (torch.cat([head, text, r(9)])[None], None)
    reqs[11] = (torch.cat([head, text, r(15)])[None], None)
    reqs[12] = (reqs[1][0].clone(), px[3])
    reqs[13] = (torch.cat([torch.tensor([1]), r(30)])[None], None)
    return [(ids, p, BUDGETS[i]) for i, (ids, p) in enumerate(reqs)]


def _expected_rows(cfg, reqs, image_of, min_shared=16):
    """the plan rules of DESIGN.md section 7e applied to this queue with an ample pool, written out on Python lists: -> (P, vision needed)"""
    ids = [r[0][0].tolist() for r in reqs]
    n = len(ids)
    tok = cfg.img_token_id

    def match(j, c):
        m = 0
        while m < min(len(ids[j]), len(ids[c])) and ids[j][m] == ids[c][m]:
            m += 1
        if tok in ids[c] and image_of[j] != image_of[c]:
            m = min(m, ids[c].index(tok))
        return min(m, len(ids[j]) - 1)
    entries = {}                                                  # creator -> rows kept
    best = [(0, None)] * n
    for c in range(n):
        gains = [match(j, c) for j in range(c + 1, n) if match(j, c) - best[j][0] >= min_shared]
        if not gains:
            continue
        entries[c] = max(gains)
        for j in range(c + 1, n):
            u = min(match(j, c), entries[c])
            if u >= min_shared and u > best[j][0]:
                best[j] = (u, c)
    P = [b[0] for b in best]
    vision = [image_of[j] is not None and not (tok in ids[j] and max(k for k, t in enumerate(ids[j]) if t == tok) < P[j]) for j in range(n)]
    return P, vision, entries


IMAGE_OF = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, None, None, 3, None]


@pytest.mark.parametrize("which", ["tiny", "small"])
def test_share_prefix_equals_oracle_and_unshared_fp32(which):
    from tests.test_gpu_inflight import _as_dicts, _cut, _oracle
    cfg = O.cfg_tiny() if which == "tiny" else O.cfg_small()
    W = O.make_weights(cfg, seed=0)
    reqs = _queue(cfg)
    want, margin = _oracle(cfg, W, reqs)
    print(f"[prefix] {which}: smallest top-2 margin over {sum(BUDGETS)} steps = {margin:.3e}; prompt lengths {[int(r[0].shape[1]) for r in reqs]}")
    assert margin >= 1e-4, f"prompt seeds {BASE}: margin {margin:.2e} -- pick other seeds, equality of ids is not decidable here"
    P, vision, entries = _expected_rows(cfg, reqs, IMAGE_OF)
    T = [int(r[0].shape[1]) for r in reqs]
    Q = cfg.resampler.num_query_tokens
    # anchors of the derivation, by hand: the strict prefix, the other image under equal ids, the text pair, the stranger
    assert P[9] == T[0] and P[12] == 22 and P[13] == 0 and P[10] == 21 and P[11] == 21 + 24 and P[3] == P[6] == 21 + Q + 2 and not vision[3] and not vision[9]
    assert vision[0] and vision[1] and vision[2] and vision[12] and 0 in entries and 10 in entries
    if which == "small":
        assert sum(vision) == 4 and sorted(entries) == [0, 1, 2, 10]    # requests 0, 1, 2 and 12 run the vision stack
    m = make_hip_model(cfg, W, torch.float32)
    eos = sorted({int(want[r][len(want[r]) // 2]) for r in (2, 7, 11)})
    n_early = 0
    for e in (None, eos):
        exp = [_cut(t, e) for t in want]
        n_early += sum(len(a) < len(b) for a, b in zip(exp, want))
        plain = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=e)
        st0 = dict(m.last_inflight_stats)
        assert "rows_reused" not in st0 and "pool_bytes" not in st0
        for i in range(14):
            assert torch.equal(plain[i].cpu(), exp[i]), (e, i)
        for sps, graph in ((1, True), (3, True), (8, True), (1, False), (3, False), (8, False)):
            got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=e, use_graph=graph, share_prefix=True)
            st = m.last_inflight_stats
            for i in range(14):
                assert torch.equal(got[i].cpu(), exp[i]), (e, sps, graph, i, got[i].tolist(), exp[i].tolist())
            assert st["rows_reused"] == sum(P) > 0 and st["rows_computed"] == sum(T) - sum(P) and st["vision_runs"] == sum(vision) < 10, (st, P, vision)
            assert st["pool_entries"] == len(entries) and st["decode_from"] == T and st["tokens"] == sum(len(x) for x in exp)
            t = cfg.text
            assert st["pool_bytes"] == st["pool_rows"] * t.num_hidden_layers * 2 * t.hidden_size * 4 and 0 < st["pool_rows"] <= sum(entries.values())
            assert st["steps"] == st0["steps"] or sps != 3              # the same boundaries as without sharing
    assert n_early >= 2
    # a pool too small for any entry, and one for exactly the first: same ids, nobody refused
    for pool, reused in ((0, 0), (T[0], None)):
        got = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True, prefix_pool_tokens=pool)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
        st = m.last_inflight_stats
        assert st["pool_rows"] <= pool and (reused is None or st["rows_reused"] == reused) and st["rows_reused"] + st["rows_computed"] == sum(T)
    # images are compared by value: clones of the pixel tensors share exactly as the same objects do
    cl = [dict(d, pixel_values=None if d["pixel_values"] is None else d["pixel_values"].clone()) for d in _as_dicts(reqs)]
    got = m.generate_many(cl, max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)) and m.last_inflight_stats["vision_runs"] == sum(vision)
    # max_batch = 1 takes generate() per request, sharing nothing
    one = m.generate_many(_as_dicts(reqs[:3]), max_batch=1, do_sample=False, eos_token_id=None, share_prefix=True)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(one, want[:3])) and m.last_inflight_stats["rows_reused"] == 0


def test_share_prefix_sampler_path_fixed_seed_fp32():
    """the device sampler under a fixed seed: request i draws with the uniforms it draws without sharing, so the ids are the same"""
    from tests.test_gpu_inflight import _as_dicts
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    reqs = _queue(cfg)
    for kw in (dict(do_sample=True, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=3, min_new_tokens=4, eos_token_id=None),
               dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.8, eos_token_id=None),
               dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.8, eos_token_id=[7, 9, 11])):
        for sps in (2, 8):
            torch.manual_seed(21)
            want = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, **kw)
            torch.manual_seed(21)
            got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, share_prefix=True, **kw)
            assert m.last_inflight_stats["rows_reused"] > 0
            for i in range(14):
                assert torch.equal(got[i], want[i]), (kw, sps, i, got[i].tolist(), want[i].tolist())


# ------------------------------------------------------------------ 4. bf16 at the engine widths
def _shared_rows_vs_oracle(m, cfg, W, prompts, share):
    """four requests of equal length in four slots (everyone keeps its slot): the first-token logits of admission and four teacher-forced decode steps
    on the slot's prompt rows, against the fp32 oracle on the full prompt: per request [(max, mean, hip argmax, oracle argmax, oracle margin)] x 5"""
    from visualcla.modeling_visualcla import VclaCache
    T = prompts[0].shape[1]
    m._inflight_logits_tap = []
    try:
        toks = m.generate_many([dict(input_ids=p[0], max_new_tokens=5) for p in prompts], max_batch=4, do_sample=False, eos_token_id=None, share_prefix=share)
        tap = {i: lg[j].float().cpu() for reqs, lg in m._inflight_logits_tap for j, i in enumerate(reqs)}
    finally:
        m._inflight_logits_tap = None
    st = dict(m.last_inflight_stats)
    kv = m._ws["if_kv"]
    t = cfg.text
    H, d = t.num_attention_heads, t.hidden_size // t.num_attention_heads
    ctx = st["ctx_max"]
    slots_kv = kv[:t.num_hidden_layers * 2 * 4 * H * ctx * d * 2].view(torch.bfloat16).view(t.num_hidden_layers, 2, 4, H, ctx, d)
    out = []
    for i, ids in enumerate(prompts):
        own = torch.zeros(t.num_hidden_layers, 2, 1, H, ctx, d, dtype=torch.bfloat16, device=DEV)
        own[:, :, 0, :, :T] = slots_kv[:, :, i, :, :T]                  # the prompt rows admission left in slot i (request i sits in slot i)
        seen = [tap[i]]
        cache = VclaCache(own, T, ctx)
        for s in range(4):
            seen.append(m.forward(input_ids=toks[i][s:s + 1][None], past_key_values=cache, use_cache=True).logits[0, -1].float().cpu())
        with torch.no_grad():
            oc = [None] * t.num_hidden_layers
            h = O.llama_forward(O.embed_and_splice(ids, None, W, cfg), W, t, torch.ones(1, T, dtype=torch.int64), oc, 0)
            refs = [O.lm_head(h[:, -1:], W)[0, 0]]
            for s in range(4):
                e = W["text_model.model.embed_tokens.weight"][toks[i][s:s + 1].cpu()][:, None, :]
                h = O.llama_forward(e, W, t, torch.ones(1, T + s + 1, dtype=torch.int64), oc, T + s)
                refs.append(O.lm_head(h, W)[0, 0])
        rows = []
        for a, b in zip(seen, refs):
            dl = (a - b).abs()
            top2 = b.topk(2).values
            rows.append((dl.max().item(), dl.mean().item(), int(a.argmax()), int(b.argmax()), float(top2[0] - top2[1])))
        out.append(rows)
    return out, st


def test_share_prefix_bf16_engine_widths():
    """the form and the numbers of test_session_turn_bf16_engine_widths: requests admitted on rows copied from another request's pass (a 40-id head,
    24 ids of their own) against the fp32 oracle on the full prompt: max < 0.12, mean < 0.022, the oracle's argmax wherever its top-2 margin is
    >= 0.24, and no further from the oracle than the same request through generate_many() without sharing (mean <= 1.25 mean0 + 1e-3)"""
    cfg = cfg_engine_small()
    W = O.make_weights(cfg, seed=1)
    m = make_hip_model(cfg, W, torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    head = torch.randint(3, cfg.text.vocab_size - 8, (1, 40), generator=g)
    prompts = [torch.cat([head, torch.randint(3, cfg.text.vocab_size - 8, (1, 24), generator=g)], dim=1) for _ in range(4)]
    with_s, st = _shared_rows_vs_oracle(m, cfg, W, prompts, True)
    assert st["rows_reused"] == 3 * 40 and st["rows_computed"] == 64 + 3 * 24 and st["admission_passes"] == 2, st
    without, _ = _shared_rows_vs_oracle(m, cfg, W, prompts, False)
    for i in range(4):
        for s, ((mx, mean, a_hip, a_ref, margin), (mx0, mean0, *_)) in enumerate(zip(with_s[i], without[i])):
            print(f"[prefix bf16] request {i} step {s}: shared max {mx:.3e} mean {mean:.3e}; unshared max {mx0:.3e} mean {mean0:.3e}; oracle margin {margin:.3e}")
    for i in range(4):
        for s, ((mx, mean, a_hip, a_ref, margin), (mx0, mean0, *_)) in enumerate(zip(with_s[i], without[i])):
            assert mx < 0.12 and mean < 0.022, (i, s, mx, mean)
            assert margin < 0.24 or a_hip == a_ref, (i, s, a_hip, a_ref, margin)
            assert mean <= 1.25 * mean0 + 1e-3, (i, s, mean, mean0)


# ------------------------------------------------------------------ 5. neighbours keep working, refusals on the device
def test_neighbours_unchanged_by_share_prefix():
    from tests.test_gpu_inflight import _as_dicts, _requests
    cfg = O.cfg_tiny()
    m = make_hip_model(cfg, O.make_weights(cfg, seed=0), torch.float32)
    reqs = _requests(cfg)
    shared = _queue(cfg)
    ids1 = reqs[11][0].cuda()
    px, ids, _ = O.make_inputs(cfg, 1, 48, seed_ids=9)
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)

    def neighbours():
        a = m.generate(input_ids=ids1, max_new_tokens=24, do_sample=False, eos_token_id=None).cpu()
        b = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None)
        s = m.new_session()
        t1 = m.generate(input_ids=ids.cuda(), pixel_values=px.cuda(), max_new_tokens=10, do_sample=False, eos_token_id=None, session=s).cpu()
        ids2 = torch.cat([ids, t1, torch.randint(3, hi, (1, 7), generator=torch.Generator().manual_seed(3))], dim=1)
        t2 = m.generate(input_ids=ids2.cuda(), pixel_values=px.cuda(), max_new_tokens=10, do_sample=False, eos_token_id=None, session=s).cpu()
        assert m.last_session_stats["reused"] == ids.shape[1] + 9
        c = m.generate(input_ids=ids1, max_new_tokens=24, do_sample=False, eos_token_id=None, prompt_lookup_num_tokens=3).cpu()
        return [a, t1, t2, c] + [x.cpu() for x in b]
    before = neighbours()
    first = m.generate_many(_as_dicts(shared), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True)
    assert m.last_inflight_stats["rows_reused"] > 0
    after = neighbours()
    again = m.generate_many(_as_dicts(shared), max_batch=4, do_sample=False, eos_token_id=None, share_prefix=True)
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_share_prefix_refusals_on_the_device():
    from tests.test_gpu_inflight import _as_dicts
    cfg = O.cfg_tiny()
    W = O.make_weights(cfg, seed=0)
    m = make_hip_model(cfg, W, torch.float32)
    reqs = _as_dicts(_queue(cfg))
    want = m.generate_many(reqs, max_batch=4, do_sample=False, eos_token_id=None, max_new_tokens=3)
    m._inflight_logits_tap = []                                         # anything admitted would leave its logits here
    masked = [dict(r) for r in reqs]
    masked[5]["attention_mask"] = torch.ones_like(reqs[5]["input_ids"])
    masked[5]["attention_mask"][0] = 0
    masked[2]["attention_mask"] = torch.ones_like(reqs[2]["input_ids"])          # all ones: no mask
    with pytest.raises(ValueError, match=r"share_prefix=True with an attention_mask.*request 5\)"):
        m.generate_many(masked, max_batch=4, do_sample=False, share_prefix=True)
    m.image_at_head = True
    with pytest.raises(ValueError, match=r"num_beams=2.*image_at_head=True"):
        m.generate_many(reqs, max_batch=4, num_beams=2, share_prefix=True)
    m.image_at_head = False
    assert m._inflight_logits_tap == []
    m._inflight_logits_tap = None
    masked[5].pop("attention_mask")
    got = m.generate_many(masked, max_batch=4, do_sample=False, eos_token_id=None, max_new_tokens=3, share_prefix=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    ecfg = cfg_engine_small()
    m16 = make_hip_model(ecfg, O.make_weights(ecfg, seed=3), torch.bfloat16)
    m16.enable_fp8_decode(True, prefill=False, kv_cache=True)
    m16._inflight_logits_tap = []
    with pytest.raises(ValueError, match="e4m3"):
        m16.generate_many([dict(input_ids=torch.arange(3, 40)), dict(input_ids=torch.arange(3, 50))], max_batch=4, do_sample=False, share_prefix=True)
    assert m16._inflight_logits_tap == []

"""The attention kernels at their seams, with a key that matters (tests/attention_probe.py): one key row gets K = 0 and a constant value
row large enough to move every output that sees it by ten times the bound, at any context; it is planted on both sides of every batch /
tile / split seam, at the clamp target, as the new token, under a zero of the key mask and in the stale rows past the position.  The
reference is a float64 softmax over exactly the visible keys.  Every test asserts the label of the launch (vcla_debug_last_launch), so it
cannot silently stop reaching the instantiation it was written for.
tests/test_attention_probe_host.py shows on the CPU that the checker rejects a wrong kernel at every (context, j) used here."""
import pytest
import torch

from tests import attention_probe as P
from tests.helpers import report as _report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KV_FP8 = 0x100     # include/visualcla_hip.h VCLA_KV_FP8
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = {"bf16": BF16, "f32": F32}


@pytest.fixture(scope="module")
def lib():
    from visualcla import _lib
    _lib.require_device()
    return _lib


def _note(rec: P.Record):
    for line in rec.lines():
        print("[attention_seams] " + line)
        _report("attention_seams " + line)


def _swap_rows(t, bi, ji, val):
    """t[bi[k], :, ji[k]] = val[k] for every k; -> the rows as they were"""
    old = t[bi, :, ji].clone()
    t[bi, :, ji] = val
    return old


def _e4m3_bytes(x):
    """the e4m3fn bytes of a float tensor (the cache is handled as uint8: indexing stays on a plain integer type)"""
    return x.float().to(torch.float8_e4m3fn).view(torch.uint8)


def _e4m3_values(b):
    return b.view(torch.float8_e4m3fn).float()


def _rope(x, cos, sin, pos, dt):
    """rotate-half RoPE with the kernels' roundings: x [B, H, d] (values of dt), pos [B] -> fp32"""
    h = x.shape[-1] // 2
    c = cos[pos].to(dt).float()[:, None, :]
    s = sin[pos].to(dt).float()[:, None, :]
    a, b = x[..., :h].float(), x[..., h:].float()
    return torch.cat([(a * c - b * s).to(dt).float(), (b * c + a * s).to(dt).float()], dim=-1)


# ================================================================== C.2 decode
def _decode_case(lib, case):
    """one case of P.flash_cases() / P.phased_cases()"""
    from visualcla.weights import rope_tables
    d, B, H, ctx_max, masked, label = (case[k] for k in ("d", "B", "H", "ctx_max", "masked", "label"))
    kv8, qp, rows, misalign = (case[k] for k in ("kv8", "qp", "rows", "misalign"))
    dtype = DTYPES[case["dtype"]]
    L = lib.load()
    g = torch.Generator(device=DEV).manual_seed(d + 3 * B + 5 * H + ctx_max + 7 * masked + 11 * kv8 + 13 * qp + 17 * rows)
    randn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    cos, sin = (t.to(DEV) for t in rope_tables(ctx_max, d, 10000.0))
    scale, HD = d ** -0.5, H * d
    atol = P.atol_of(case["dtype"])
    vmax = P.E4M3_MAX if kv8 else None
    enc = _e4m3_bytes if kv8 else (lambda x: x.to(dtype))          # a value -> what the cache stores
    dec = _e4m3_values if kv8 else (lambda x: x.float())
    batch_keys = P.decode_batch_keys(case)
    kc, vc = enc(randn(B, H, ctx_max, d)), enc(randn(B, H, ctx_max, d))
    assert kc.numel() * kc.element_size() <= 256 << 20
    K64, V64 = dec(kc).double(), dec(vc).double()        # the reference reads the dequantised cache
    if qp:       # the qkv row arrives as two raw fp32 K slices; the kernel sums them and rounds to bf16
        parts0 = randn(2, B, 3 * HD) * 0.5 ** 0.5          # the sum of the slices is N(0, 1), as the plant's weight assumes
        parts = parts0.clone()
        qkv0 = (parts0[0] + parts0[1]).to(BF16).view(B, 3, H, d)
    else:
        qkv0 = randn(B, 3, H, d).to(BF16).to(dtype)
    qkv = qkv0.clone()
    obuf = torch.zeros(B * HD + 8, dtype=dtype, device=DEV)
    out = obuf[4:4 + B * HD] if misalign else obuf[:B * HD]
    assert (out.data_ptr() % 16 != 0) == misalign
    arB = torch.arange(B, device=DEV)
    ar = torch.arange(ctx_max, device=DEV)
    code = lib.dtype_code(dtype) | (KV_FP8 if kv8 else 0)
    if rows:     # one launch, every row at its own position: all the positions, one row inactive, one at ctx_max - 1
        contexts = [torch.tensor(P.decode_row_positions(case), dtype=torch.int32, device=DEV)]
    else:
        contexts = [torch.full((B,), p, dtype=torch.int32, device=DEV) for p in P.decode_positions(ctx_max)]
    rec = P.Record()

    for pos_rows in contexts:
        active = pos_rows >= 0
        pidx = pos_rows.clamp(min=0).long()
        tag = f"decode {label} ctx_max={ctx_max} pos={'rows' if rows else int(pos_rows[0])}"
        km = None
        pos_list = pos_rows.tolist()
        if masked:   # zeros in the first batch and three keys before the position
            km = torch.ones(B, ctx_max, dtype=torch.int32, device=DEV)
            for b, p in enumerate(pos_list):
                for j in P.decode_masked_keys(p):
                    km[b, j] = 0
        vis = (ar[None, :] <= pos_rows[:, None].long())
        if km is not None:
            vis = vis & (km != 0)
        vis4 = vis[:, None, None, :]
        c_rows = torch.tensor([P.plant_value(p + 1, vmax) for p in pos_list], device=DEV)

        def launch():
            out.zero_()
            kmp, ld = (km.data_ptr(), ctx_max) if km is not None else (None, 0)
            if rows:
                lib.check(L.vcla_attn_decode_rows(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), B, H, d,
                                                  ctx_max, pos_rows.data_ptr(), kmp, ld, scale, code, 0, lib.stream_ptr()))
                return out.view(B, H, d).clone()
            pos = int(pos_rows[0])
            dev_part = min(2, pos)               # position = pos0 + *pos_dev
            pos_dev = torch.tensor([dev_part], dtype=torch.int32, device=DEV)
            if qp:
                lib.check(L.vcla_attn_decode_fused_parts(parts.data_ptr(), B * 3 * HD, None, None, 1e-6, kc.data_ptr(), vc.data_ptr(), cos.data_ptr(),
                                                         sin.data_ptr(), out.data_ptr(), B, H, d, ctx_max, pos - dev_part, pos_dev.data_ptr(), kmp, ld,
                                                         scale, code, 0, lib.stream_ptr()))
            else:
                lib.check(L.vcla_attn_decode_fused(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), B, H, d,
                                                   ctx_max, pos - dev_part, pos_dev.data_ptr(), kmp, ld, scale, code, 0, lib.stream_ptr()))
            return out.view(B, H, d).clone()

        def new_rows(q3):
            """what the kernel appends at the position: the roped key and the value of the qkv row, in the cache's precision"""
            kn, vn = _rope(q3[:, 1], cos, sin, pidx, dtype), q3[:, 2].float()
            return dec(enc(kn)).double(), dec(enc(vn)).double()

        q64 = _rope(qkv0[:, 0], cos, sin, pidx, dtype).double()[:, :, None, :]
        kn, vn = new_rows(qkv0)
        saved = [t[arB, :, pidx].clone() for t in (kc, vc, K64, V64)]        # the row at the position: the kernel overwrites it
        K64[arB, :, pidx], V64[arB, :, pidx] = kn, vn

        base = launch()
        assert lib.last_launch() == label, lib.last_launch()
        ref0 = P.reference(q64, K64, V64, scale, vis4)[:, :, 0]
        err0 = ((base.double() - ref0).abs() / (atol + P.REL * ref0.abs()))[active].max().item()
        assert err0 <= 1.0 and torch.isfinite(base.float()).all(), f"{tag}: the unplanted run is {err0:.2f} x the bound from the reference"
        assert not base[~active].any(), f"{tag}: an inactive row is not zero"

        def plant(j_rows, name, must_see):
            on = active & (j_rows >= 0) & (j_rows <= pos_rows)
            cached, newtok = on & (j_rows < pos_rows), on & (j_rows == pos_rows)
            bi, ji = arB[cached], j_rows[cached].long()
            cv = c_rows[cached][:, None, None].expand(-1, H, d)
            olds = [_swap_rows(kc, bi, ji, 0), _swap_rows(vc, bi, ji, enc(cv)), _swap_rows(K64, bi, ji, 0.0), _swap_rows(V64, bi, ji, cv.double())]
            if newtok.any():
                qkv[newtok, 1] = 0.0
                qkv[newtok, 2] = c_rows[newtok][:, None, None].expand(-1, H, d).to(qkv.dtype)
                if qp:
                    pv = parts.view(2, B, 3, H, d)
                    pv[:, newtok, 1] = 0.0
                    pv[1, newtok, 2] = 0.0
                    pv[0, newtok, 2] = c_rows[newtok][:, None, None].expand(-1, H, d)
                kn2, vn2 = new_rows(qkv)
                K64[arB, :, pidx], V64[arB, :, pidx] = kn2, vn2
            got = launch()
            ref = P.reference(q64, K64, V64, scale, vis4)[:, :, 0]
            sees = (on & vis[arB, j_rows.clamp(min=0).long()])[:, None].expand(B, H)
            assert bool(sees.any()) == must_see, (name, j_rows)
            m = P.check(f"{tag} {name}", got, ref, base, sees, atol)
            if must_see:
                rec.add(tag, m)
            for t, o in zip((kc, vc, K64, V64), olds):
                t[bi, :, ji] = o
            if newtok.any():
                qkv.copy_(qkv0)
                if qp:
                    parts.copy_(parts0)
                K64[arB, :, pidx], V64[arB, :, pidx] = kn, vn

        def rows_of(js):
            return torch.tensor(js, dtype=torch.int32, device=DEV)

        if rows:     # every row takes the same KIND of plant at its own position; a kind a row has no visible key for falls on its new token
            for kind, v in P.decode_kinds(batch_keys):
                js = [P.decode_kind_plant(kind, v, p, masked) if p >= 0 else -1 for p in pos_list]
                plant(rows_of([p if j is None else j for j, p in zip(js, pos_list)]), f"j={kind}{v:+d}", True)
        else:
            for j in P.decode_plants(pos_list[0], batch_keys, masked):
                plant(torch.full_like(pos_rows, j), f"j={j}", True)
        if masked:       # rule c: a plant under a zero of the mask moves nothing
            for i in range(2):
                js = [P.decode_masked_keys(p)[i] if p >= 0 and P.decode_masked_keys(p) else -1 for p in pos_list]
                if max(js) >= 0:
                    plant(rows_of(js), f"masked key {i}", False)
        # rule c: the stale rows pos + 1 .. pos + 3 hold K = 0 and a huge V
        olds = []
        for k in (1, 2, 3):
            ok = active & (pos_rows + k < ctx_max)
            bi, ji = arB[ok], (pos_rows[ok] + k).long()
            sv = enc(torch.full((1,), min(P.STALE_VALUE, vmax or P.STALE_VALUE), device=DEV))
            olds.append((bi, ji, _swap_rows(kc, bi, ji, 0), _swap_rows(vc, bi, ji, sv)))
        got = launch()
        P.check(f"{tag} stale rows", got, ref0, base, torch.zeros(B, H, dtype=torch.bool, device=DEV), atol)
        for bi, ji, ok_, ov_ in olds:
            kc[bi, :, ji], vc[bi, :, ji] = ok_, ov_
        for t, o in zip((kc, vc, K64, V64), saved):
            t[arB, :, pidx] = o
    _note(rec)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in P.flash_cases()])
def test_decode_flash_planted_keys(lib, case):
    """attn_decode_flash_kernel, every instantiation launch_decode selects: the batch seams of the A / B register buffers (U * KPB keys), the
    clamp target pos - 1, the new token, the mask, the stale rows"""
    _decode_case(lib, case)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["label"]) for c in P.phased_cases()])
def test_decode_phased_planted_keys(lib, case):
    """attn_decode_kernel (fp32, and bf16 when the output is not 16-byte aligned), one key per thread and row-cooperative: the pass seams of
    the score and the P V loops (UV * KPB keys), the new token, the mask, the stale rows"""
    _decode_case(lib, case)


# ================================================================== C.3 verify
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("R,ctx_max", P.VERIFY_CASES)
def test_verify_planted_keys(lib, dtype, masked, R, ctx_max):
    """vcla_attn_verify: the KT = 32 tile seam, every split seam (S and the split length from the scratch size), p - 1, the new rows p, p + 1 and
    p + R - 1 (row i of the pass sees the new row p + i' only for i' <= i), the mask, the stale rows"""
    L = lib.load()
    H, d, dt = 4, 128, DTYPES[dtype]
    g = torch.Generator(device=DEV).manual_seed(R + ctx_max + 3 * masked)
    randn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    from visualcla.weights import rope_tables
    cos, sin = (t.to(DEV) for t in rope_tables(ctx_max, d, 10000.0))
    scale = d ** -0.5
    atol = P.atol_of(dtype, wide=True)
    nb = L.vcla_attn_verify_scratch_bytes(H, d, ctx_max)
    S = nb // (H * 16 * (d + 2) * 4) if nb else 1
    assert S == P.verify_splits(ctx_max) and (S > 1) == (ctx_max > 256)
    label = "attn_verify_merge_kernel" if S > 1 else "attn_verify_kernel<S=1>"      # the merge launch runs only behind attn_verify_kernel<split>
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    kv0 = randn(2, H, ctx_max, d).to(dt)
    rec = P.Record()
    for p in P.verify_contexts(R, ctx_max):
        N = p + R
        tag = f"verify {dtype} d={d} R={R} masked={int(masked)} ctx_max={ctx_max} p={p}"
        qkv0 = randn(R, 3, H, d).to(BF16).to(dt)
        km = None
        if masked:
            km = torch.ones(1, ctx_max, dtype=torch.int32, device=DEV)
            for j in P.verify_masked_keys(p):
                km[0, j] = 0
        qpos = torch.arange(p, p + R, device=DEV)
        vis = P.causal_visible(qpos, N, km[0] if masked else None)          # [R, N]
        c = P.plant_value(N)

        def run(qkv, kv):
            out = torch.zeros(R, H * d, dtype=dt, device=DEV)
            lib.check(L.vcla_attn_verify(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), R, H, d, ctx_max,
                                         p, None, lib.ptr(km), scale, lib.dtype_code(dt), 0, scratch.data_ptr(), scratch.numel(), lib.stream_ptr()))
            return out.view(R, H, d)

        def ref_of(qkv, kv):
            """float64 attention of the R rows over the cache rows [0, p) and the R new rows"""
            q = _rope(qkv[:, 0], cos, sin, qpos, dt).double().transpose(0, 1)                      # [H, R, d]
            K = torch.cat([kv[0, :, :p].double(), _rope(qkv[:, 1], cos, sin, qpos, dt).double().transpose(0, 1)], dim=1)
            V = torch.cat([kv[1, :, :p].double(), qkv[:, 2].double().transpose(0, 1)], dim=1)
            return P.reference(q, K, V, scale, vis).transpose(0, 1)                                 # [R, H, d]

        base = run(qkv0, kv0.clone())
        assert lib.last_launch() == label, lib.last_launch()
        ref0 = ref_of(qkv0, kv0)
        err0 = ((base.double() - ref0).abs() / (atol + P.REL * ref0.abs())).max().item()
        assert err0 <= 1.0, f"{tag}: the unplanted run is {err0:.2f} x the bound from the reference"
        for j in P.verify_plants(p, R, S, masked) + (list(P.verify_masked_keys(p)) if masked else []):
            kv, qkv = kv0.clone(), qkv0.clone()
            if j < p:
                kv[0, :, j], kv[1, :, j] = 0.0, c
            else:
                qkv[j - p, 1], qkv[j - p, 2] = 0.0, c
            got = run(qkv, kv)
            sees = vis[:, j][:, None].expand(R, H)
            m = P.check(f"{tag} j={j}", got, ref_of(qkv, kv), base, sees, atol)
            if sees.any():
                rec.add(tag, m)
            else:
                assert masked and j in P.verify_masked_keys(p)
        kv = kv0.clone()
        kv[0, :, N:N + 3], kv[1, :, N:N + 3] = 0.0, P.STALE_VALUE
        P.check(f"{tag} stale rows", run(qkv0, kv), ref0, base, torch.zeros(R, H, dtype=torch.bool, device=DEV), atol)
    _note(rec)


# ================================================================== C.4 MFMA prefill and the ViT forms
def _qkv_views(qkv):
    """fused [B, T, 3, H, D] -> q, k, v [B, H, T, D] views (the strided layout the model issues)"""
    return tuple(qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def _attend(lib, q, k, v, causal, km, fk, misalign=False):
    B, H, Tq, D = q.shape
    buf = torch.zeros(B * Tq * H * D + 8, dtype=BF16, device=DEV)
    out = (buf[4:-4] if misalign else buf[:-8]).view(B, Tq, H * D)
    assert (out.data_ptr() % 16 != 0) == misalign
    lib.attention(q, k, v, D ** -0.5, causal=causal, key_mask=km, out=out, force_kernel=fk)
    return out.view(B, Tq, H, D)


def _attend_ref(q, k, v, causal, km):
    """-> [B, Tq, H, D] float64"""
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    vis = torch.ones(1, 1, Tq, Tk, dtype=torch.bool, device=q.device)
    if causal:
        vis = P.causal_visible(torch.arange(Tq, device=q.device) + (Tk - Tq), Tk)[None, None]
    if km is not None:
        vis = vis & (km[:, None, None, :Tk] != 0)
    return P.reference(q, k, v, D ** -0.5, vis).transpose(1, 2)


MFMA_PARITY = [
    # the whole prompt in LDS (causal prefill at B = 64, T = 128): two tiles, two tiles with a ragged end and left padding, one tile
    ("attn_mfma_kernel<128, 4, 2>", 2, (16, 32, 128, 128, 128, True), False, False),
    ("attn_mfma_kernel<128, 4, 2>", 2, (16, 32, 100, 100, 128, True), True, False),
    ("attn_mfma_kernel<128, 4, 2>", 2, (16, 32, 64, 64, 128, True), False, False),
    # 9 waves per workgroup: B * H >= 256 and more than 128 query rows
    ("attn_mfma_kernel<64, 9, 0>", 2, (16, 16, 257, 257, 64, False), False, False),
    ("attn_mfma_kernel<64, 9, 0>", 2, (16, 16, 200, 321, 64, False), False, False),
    ("attn_mfma_kernel<64, 9, 0>", 2, (16, 16, 257, 257, 64, False), True, False),        # a key mask: no remainder peel
    # the other forms the dispatcher selects
    ("attn_mfma_kernel<64, 4, 0>", 2, (2, 3, 257, 257, 64, False), False, False),
    ("attn_mfma_kernel<64, 2, 0>", 2, (2, 1, 33, 64, 64, False), False, False),
    ("attn_mfma_kernel<128, 4, 0>", 2, (1, 2, 130, 130, 128, True), False, False),
    # the register-staged ViT kernel, selected because the output is not 16-byte aligned (no environment variable), and the other ViT forms
    ("attn_vit_kernel<4>", 3, (3, 2, 257, 257, 64, False), False, True),
    ("attn_vit_dma_kernel", 3, (3, 2, 257, 257, 64, False), False, False),
    ("attn_vit_kernel<1>", 3, (2, 4, 65, 65, 64, False), False, False),
    ("attn_vit_long_kernel<9>", 3, (2, 3, 577, 577, 64, False), False, False),
]


@pytest.mark.parametrize("label,fk,shape,masked,misalign", MFMA_PARITY, ids=[f"{m[0]}-{'x'.join(map(str, m[2]))}-m{int(m[3])}" for m in MFMA_PARITY])
def test_attention_mfma_instantiations(lib, label, fk, shape, masked, misalign):
    """random-input parity of the form of test_attention_mfma at shapes that reach every instantiation vcla_attention_mfma / _vit selects"""
    B, H, Tq, Tk, D, causal = shape
    g = torch.Generator(device=DEV).manual_seed(B * 3 + H + Tq + Tk + D)
    if Tq == Tk:
        q, k, v = _qkv_views(torch.randn(B, Tq, 3, H, D, generator=g, device=DEV).to(BF16))
    else:
        q, k, v = (torch.randn(B, H, T, D, generator=g, device=DEV).to(BF16) for T in (Tq, Tk, Tk))
    km, valid = None, torch.ones(B, Tq, dtype=torch.bool, device=DEV)
    if masked:
        km = torch.ones(B, Tk, dtype=torch.int32, device=DEV)
        km[1, :9] = 0                                   # left padding
        if causal:
            valid[1, :9] = False                        # rows whose every visible key is masked are don't-care
        else:
            km[2, 70:75] = 0
    got = _attend(lib, q, k, v, causal, km, fk, misalign)
    assert lib.last_launch() == label, lib.last_launch()
    ref = _attend_ref(q, k, v, causal, km)
    assert torch.isfinite(got.float()).all()
    err = (got.double() - ref).abs()[valid].max().item()
    _report(f"attn_mfma_instantiations[{label},{shape},mask{int(masked)}]: max_abs_err={err:.3e}")
    assert err <= (P.ATOL_BF16_WIDE if fk == 3 else P.ATOL_BF16), f"{label} {shape}: max err {err:.3e}"


@pytest.mark.parametrize("label,B,H,T", P.CAUSAL_CASES)
def test_prefill_causal_planted_keys(lib, label, B, H, T):
    """causal d = 128 prefill: rows below j are bit-identical to the base run, row j (the diagonal) and the rows after it see the plant"""
    D = 128
    g = torch.Generator(device=DEV).manual_seed(T + B)
    qkv0 = torch.randn(B, T, 3, H, D, generator=g, device=DEV).to(BF16)
    q, k, v = _qkv_views(qkv0)
    base = _attend(lib, q, k, v, True, None, 2)
    assert lib.last_launch() == label, lib.last_launch()
    rec, c = P.Record(), P.plant_value(T)
    for j in P.PREFILL_CAUSAL[T]:
        qkv = qkv0.clone()
        qkv[:, j, 1], qkv[:, j, 2] = 0.0, c
        q, k, v = _qkv_views(qkv)
        got = _attend(lib, q, k, v, True, None, 2)
        sees = (torch.arange(T, device=DEV) >= j)[None, :, None].expand(B, T, H)
        rec.add(f"prefill {label} T={T}", P.check(f"prefill {label} T={T} j={j}", got, _attend_ref(q, k, v, True, None), base, sees, P.ATOL_BF16))
    _note(rec)


@pytest.mark.parametrize("label,fk,B,H,Tq,Tk,misalign", P.BIDIR_CASES, ids=[f"{m[0]}-{m[4]}x{m[5]}" for m in P.BIDIR_CASES])
def test_bidirectional_planted_keys(lib, label, fk, B, H, Tq, Tk, misalign):
    """bidirectional d = 64 at 257 / 321 / 577 keys: the first key, both sides of the first tile seam, and key Tk - 1 -- the remainder key the MFMA
    kernel peels off the tile loop, the 257th / 577th key the ViT forms take on the VALU"""
    D = 64
    g = torch.Generator(device=DEV).manual_seed(Tq + Tk + B)
    q0 = torch.randn(B, H, Tq, D, generator=g, device=DEV).to(BF16)
    kv0 = torch.randn(2, B, H, Tk, D, generator=g, device=DEV).to(BF16)
    if Tq == Tk:      # the fused layout (the ViT forms require nothing of it, the model issues it)
        fused = torch.stack([q0, kv0[0], kv0[1]], dim=0).permute(1, 3, 0, 2, 4).contiguous()       # [B, T, 3, H, D]
        q0, k0, v0 = _qkv_views(fused)
    else:
        k0, v0 = kv0[0], kv0[1]
    atol = P.atol_of("bf16", wide=fk == 3)
    base = _attend(lib, q0, k0, v0, False, None, fk, misalign)
    assert lib.last_launch() == label, lib.last_launch()
    rec, c = P.Record(), P.plant_value(Tk)
    sees = torch.ones(B, Tq, H, dtype=torch.bool, device=DEV)
    for j in P.PREFILL_BIDIR[Tk]:
        old = k0[:, :, j].clone(), v0[:, :, j].clone()
        k0[:, :, j], v0[:, :, j] = 0.0, c
        got = _attend(lib, q0, k0, v0, False, None, fk, misalign)
        rec.add(f"bidirectional {label} {Tq}x{Tk}", P.check(f"bidirectional {label} {Tq}x{Tk} j={j}", got, _attend_ref(q0, k0, v0, False, None), base, sees, atol))
        k0[:, :, j], v0[:, :, j] = old
    _note(rec)

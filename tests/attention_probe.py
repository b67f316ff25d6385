"""The planted-key probe shared by the attention tests (tests/test_gpu_attention_seams.py, tests/test_attention_probe_host.py).

With N(0, 1) keys and values a softmax over n keys gives each key a weight of about 1 / n and the output is an average of n random
rows: one key lost among 1900 moves a bf16 output by 0.004, far inside the 1.5e-2 the random-input tests allow.  The probe makes ONE key
matter at any context:

  the plant    key row j gets K = 0 (score 0 whatever q is; RoPE of 0 is 0) and the constant value row c = bf16(max(4, (n + 1) / 4)),
               n = the number of visible keys.  Its weight is about 1 / (1.65 n) (E exp(s) = e^0.5 for s ~ N(0, 1)), so it adds about
               0.15 to every output element of every row that sees it -- ten times the bound, at any n.
  the reference  a float64 softmax over exactly the visible keys.
  the checker  for one (kernel, context, j):
               a. every row that may see j agrees with the reference within atol + 2^-7 |ref| (atol = the bound of the kernel's
                  random-input test; 2^-7 = two bf16 roundings, the probabilities and the output);
               b. every row that may see j differs from the unplanted base run by more than twice that bound;
               c. every row that must not see j (causally earlier, masked out, a stale row past the position) is bit-identical to
                  the base run.

The module also holds the (context, j) tables of the GPU tests, so that the host test can show the checker rejecting a wrong kernel at
every one of them."""
import math
from typing import NamedTuple

import torch

REL = 2.0 ** -7
ATOL_BF16 = 1.5e-2          # test_attention_mfma / test_attn_decode_fused
ATOL_BF16_WIDE = 2e-2       # test_attention_vit_whole_sequence / test_verify_attention_vs_torch_and_decode
ATOL_F32 = 3e-5             # test_attn_decode_fused
STALE_VALUE = 1e4           # what the rows past the position are filled with (K = 0): seen once, it moves every element by ~ 1e4 / n
E4M3_MAX = 448.0


def plant_value(n: int, vmax: float = None) -> float:
    """the constant of the planted value row for n visible keys, a bf16 value (vmax: the largest value the cache format holds)"""
    c = max(4.0, 0.25 * (n + 1))
    if vmax is not None:
        c = min(c, vmax)
    return float(torch.tensor(c, dtype=torch.float32).to(torch.bfloat16))


def reference(q, K, V, scale, visible):
    """float64 softmax over exactly the visible keys.  q [..., R, d], K / V [..., N, d], visible bool broadcastable to [..., R, N]
    -> [..., R, d] float64; a row that sees nothing is 0"""
    s = torch.einsum("...rd,...jd->...rj", q.double(), K.double()) * scale
    s = s.masked_fill(~visible, float("-inf"))
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)
    return torch.einsum("...rj,...jd->...rd", p, V.double())


def causal_visible(qpos, n_keys, key_mask=None):
    """[R, N]: key j is visible to the query at position qpos[i] iff j <= qpos[i] and its mask entry is not 0"""
    qpos = torch.as_tensor(qpos)
    vis = torch.arange(n_keys, device=qpos.device)[None, :] <= qpos[:, None]
    if key_mask is not None:
        vis = vis & (key_mask[:n_keys] != 0)[None, :]
    return vis


class Measure(NamedTuple):
    err: float      # worst |got - ref| / bound over the rows that may see the plant (rule a holds iff <= 1)
    move: float     # smallest over those rows of the row's largest |got - base| / bound (rule b holds iff > 2)
    leak: float     # largest |got - base| / bound over the rows that must not see it; rule c wants 0 AND equal bits
    same_bits: bool


def measure(got, ref, base, sees, atol) -> Measure:
    """got / base [..., d] as the kernel stored them (same dtype), ref [..., d] float64, sees bool [...]: the rows that may see the plant"""
    assert got.shape == ref.shape == base.shape and sees.shape == got.shape[:-1], (got.shape, ref.shape, base.shape, sees.shape)
    g, b, r = got.double(), base.double(), ref.double()
    bound = atol + REL * r.abs()
    err = ((g - r).abs() / bound)[sees]
    move = ((g - b).abs() / bound).amax(dim=-1)[sees]
    leak = ((g - b).abs() / bound)[~sees]
    finite = bool(torch.isfinite(g).all())
    return Measure(err=float(err.max()) if err.numel() and finite else (0.0 if finite else math.inf),
                   move=float(move.min()) if move.numel() else math.inf,
                   leak=float(leak.max()) if leak.numel() else 0.0,
                   same_bits=torch.equal(got[~sees], base[~sees]))


def check(name, got, ref, base, sees, atol) -> Measure:
    """the three rules; returns the measurement for the record"""
    m = measure(got, ref, base, sees, atol)
    assert m.err <= 1.0, f"{name}: rule a: a row that may see the plant is {m.err:.2f} x the bound (atol {atol} + 2^-7 |ref|) from the reference"
    assert m.move > 2.0, f"{name}: rule b: a row that may see the plant moved only {m.move:.2f} x the bound from the base run"
    assert m.same_bits, f"{name}: rule c: a row that must not see the plant differs from the base run ({m.leak:.2f} x the bound)"
    return m


class Record:
    """worst error / bound and smallest move / bound per (kernel, context), for profiles/attention_seams.txt"""

    def __init__(self):
        self.rows = {}

    def add(self, key, m: Measure):
        e, v, n = self.rows.get(key, (0.0, math.inf, 0))
        self.rows[key] = (max(e, m.err), min(v, m.move), n + 1)

    def lines(self):
        return [f"{k}: plants {n} worst err/bound {e:.3f} smallest move/bound {v:.2f}" for k, (e, v, n) in self.rows.items()]


# ------------------------------------------------------------------ the cases and (context, j) tables of the GPU tests
# tests/test_gpu_attention_seams.py runs exactly these; tests/test_attention_probe_host.py derives its parametrisation from the same
# functions, so the two cannot drift apart.
def atol_of(dtype, wide=False):
    """the bound of the kernel's existing random-input test (dtype: "bf16" / "f32"; wide: the verify and ViT kernels' 2e-2)"""
    return ATOL_F32 if dtype == "f32" else (ATOL_BF16_WIDE if wide else ATOL_BF16)


DECODE_POSITIONS = (0, 1, 37, 700, 1023, 1900)        # and ctx_max - 1


def decode_positions(ctx_max):
    return [p for p in DECODE_POSITIONS if p < ctx_max - 1] + [ctx_max - 1]


def flash_batch_keys(d, nw, kv8=False):
    """keys per batch of attn_decode_flash_kernel, U * KPB (E, LPK, KPW, U as in the kernel): the A / B register buffers alternate by it"""
    E = 16 if kv8 else 8
    LPK = d // E
    KPB = nw * (64 // LPK)
    U = (4 if nw == 2 else 8) // (2 if kv8 else 1)
    return U * KPB


def phased_batch_keys(d, nw):
    """keys per pass of attn_decode_kernel's P V loop (and of its row-cooperative score loop): UV * KPB"""
    return 8 * nw * (64 // (d // 8))


def _tf(b):
    return "true" if b else "false"


def flash_cases():
    """one case per instantiation of attn_decode_flash_kernel that launch_decode selects (B * H >= 1024 selects the 2-wave form)"""
    cases = []
    for d in (128, 64, 32):
        for nw in (4, 2):
            B, H, ctx_max = ((2, 3, 2048) if d != 128 else (1, 2, 2048)) if nw == 4 else (32, 32, 1024)
            for masked in (False, True):
                for kv8, qp, rows in ((False, False, False), (True, False, False), (False, False, True), (False, True, False), (True, True, False)):
                    if (kv8 or qp) and d == 32:        # the e4m3 cache and the split qkv row need d >= 64
                        continue
                    if qp and nw != 2:                 # the split qkv row exists only in the 2-wave form
                        continue
                    label = f"attn_decode_flash_kernel<D={d},NW={nw},MASK={_tf(masked)},KV8={_tf(kv8)},QP={_tf(qp)},ROWS={_tf(rows)}>"
                    cases.append(dict(kernel="flash", d=d, B=max(B, 8) if rows else B, H=H, ctx_max=ctx_max, dtype="bf16", masked=masked, label=label,
                                      kv8=kv8, qp=qp, rows=rows, misalign=False, nw=nw))
    return cases


def phased_cases():
    """attn_decode_kernel: fp32, and bf16 with an output that is not 16-byte aligned; one key per thread (B * H < 512), row-cooperative with 4 waves
    and, at d = 128 and B * H >= 1024, with 2.  fp32 caches stay within 256 MiB: that forces ctx_max = 512 on the fp32 2-wave form only."""
    cases = []
    for dtype in ("f32", "bf16"):
        for d in (128, 64, 32):
            for coop, nw in ((False, 4), (True, 4), (True, 2)):
                if nw == 2 and d != 128:
                    continue
                for rows in (False, True):
                    if not coop:
                        B, H, ctx_max = (8 if rows else 2), 3, 2048
                    elif nw == 4:
                        B, H, ctx_max = 16, 32, (1024 if d == 128 or dtype == "f32" else 2048)
                    else:
                        B, H, ctx_max = 32, 32, (512 if dtype == "f32" else 1024)
                    label = f"attn_decode_kernel<{dtype},D={d},COOP={_tf(coop)},NW={nw},ROWS={_tf(rows)}>"
                    cases.append(dict(kernel="phased", d=d, B=B, H=H, ctx_max=ctx_max, dtype=dtype, masked=(d != 64) != rows, label=label, kv8=False,
                                      qp=False, rows=rows, misalign=dtype == "bf16", nw=nw))
    return cases


def decode_batch_keys(case):
    return flash_batch_keys(case["d"], case["nw"], case["kv8"]) if case["kernel"] == "flash" else phased_batch_keys(case["d"], case["nw"])


def decode_row_positions(case):
    """ROWS: the position of every row of the one launch -- all the positions, one row inactive (-1), one at ctx_max - 1"""
    plist = decode_positions(case["ctx_max"]) + [-1]
    assert case["B"] >= len(plist)
    return [plist[b % len(plist)] for b in range(case["B"])]


def decode_masked_keys(pos):
    """the zeros of the key mask: one in the first batch, one three keys before the position"""
    return (2, pos - 3) if pos > 8 else ()


def decode_kinds(batch_keys):
    """j = 0, both sides of the first and the second batch seam (absolute), pos - 2, pos - 1 (the clamp target) and pos (the new token)"""
    return [("abs", 0), ("abs", batch_keys - 1), ("abs", batch_keys), ("abs", 2 * batch_keys - 1), ("abs", 2 * batch_keys),
            ("rel", -2), ("rel", -1), ("rel", 0)]


def decode_kind_plant(kind, v, pos, masked):
    """the key a plant of this kind falls on at `pos`, None where there is no such visible key"""
    j = v if kind == "abs" else pos + v
    if not 0 <= j <= pos or (masked and j in decode_masked_keys(pos)):
        return None
    return j


def decode_plants(pos, batch_keys, masked=False):
    """the visible plants of one position, ascending (a ROWS launch gives every row the plant of one kind, its new token where it has none)"""
    js = {decode_kind_plant(k, v, pos, masked) for k, v in decode_kinds(batch_keys)}
    return sorted(j for j in js if j is not None)


def decode_host_contexts():
    """every distinct (d, batch_keys, pos, masked, kv8, dtype) the decode cases reach"""
    out = set()
    for c in flash_cases() + phased_cases():
        positions = [p for p in decode_row_positions(c) if p >= 0] if c["rows"] else decode_positions(c["ctx_max"])
        out |= {(c["d"], decode_batch_keys(c), p, c["masked"], c["kv8"], c["dtype"]) for p in positions}
    return sorted(out)


VERIFY_CONTEXTS = (37, 700, 1900)
VERIFY_CASES = ((2, 2048), (16, 2048), (7, 256))         # (R, ctx_max); ctx_max = 256: one split, no merge launch
VERIFY_KT = 32


def verify_contexts(R, ctx_max):
    return [p for p in VERIFY_CONTEXTS if p + R + 3 <= ctx_max]


def verify_splits(ctx_max):
    """S of attn_verify_kernel (the GPU test checks it against vcla_attn_verify_scratch_bytes)"""
    return min(8, max(1, (ctx_max + 255) // 256))


def verify_split_len(p, R, S):
    """keys per split of attn_verify_kernel: the keys [0, p + R) over S splits, whole tiles of 32"""
    return ((p + R + S - 1) // S + VERIFY_KT - 1) // VERIFY_KT * VERIFY_KT


def verify_masked_keys(p):
    return (5, p - 3)


def verify_plants(p, R, S, masked=False):
    """0, both sides of a tile seam and of every split seam, p - 1, the new rows p, p + 1 and p + R - 1 (visible ones only)"""
    per = verify_split_len(p, R, S)
    js = {0, VERIFY_KT - 1, VERIFY_KT, p - 1, p, p + 1, p + R - 1}
    for s in range(1, S):
        js |= {s * per - 1, s * per}
    hidden = set(verify_masked_keys(p)) if masked else set()
    return sorted(j for j in js - hidden if 0 <= j < p + R)


def verify_host_contexts():
    return [(R, ctx_max, p, masked, dtype) for R, ctx_max in VERIFY_CASES for p in verify_contexts(R, ctx_max) for masked in (False, True)
            for dtype in ("bf16", "f32")]


# MFMA prefill / ViT (bf16).  Plants by T (causal) or Tk (bidirectional: Tk - 1 is the peeled remainder key, the 257th / 577th key of the ViT forms)
PREFILL_CAUSAL = {2048: (0, 63, 64, 127, 128, 2047), 128: (0, 63, 64, 127)}
PREFILL_BIDIR = {257: (0, 63, 64, 256), 321: (0, 63, 64, 320), 577: (0, 63, 64, 576)}
CAUSAL_CASES = [("attn_mfma_kernel<128, 4, 0>", 1, 2, 2048), ("attn_mfma_kernel<128, 4, 2>", 16, 32, 128)]        # (label, B, H, T), d = 128
BIDIR_CASES = [          # (label, force_kernel, B, H, Tq, Tk, output not 16-byte aligned), d = 64; force_kernel 3 = the ViT forms (bound 2e-2)
    ("attn_mfma_kernel<64, 9, 0>", 2, 16, 16, 257, 257, False),
    ("attn_mfma_kernel<64, 9, 0>", 2, 16, 16, 200, 321, False),
    ("attn_mfma_kernel<64, 9, 0>", 2, 16, 16, 577, 577, False),
    ("attn_mfma_kernel<64, 4, 0>", 2, 2, 3, 257, 257, False),
    ("attn_vit_dma_kernel", 3, 3, 2, 257, 257, False),
    ("attn_vit_kernel<4>", 3, 3, 2, 257, 257, True),
    ("attn_vit_long_kernel<9>", 3, 2, 3, 577, 577, False),
]

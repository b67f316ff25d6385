"""The planted-key probe bites (tests/attention_probe.py), shown on the CPU: at every (context, j) the GPU tests use -- the parametrisation is
derived from the case tables tests/test_gpu_attention_seams.py runs, masked plants and per-row positions included -- the honest reference
rounded once to bf16 passes the checker, and every deliberately wrong one -- key j dropped, counted twice, taken from row j + 1, the causal
diagonal off by one in either direction, a masked key seen, the stale row past the position seen -- is rejected in every head, by a factor
of 2 or more over the bound."""
import math

import pytest
import torch

from tests import attention_probe as P

H = 2


def _bf(t):
    return t.to(torch.bfloat16)


def _scene(seed, d, qpos, n_keys):
    """q [H, R, d], K / V [H, n_keys + 3, d] (the last three rows are stale: past every position), bf16 values"""
    g = torch.Generator().manual_seed(seed)
    q, K, V = (_bf(torch.randn(H, n, d, generator=g)).float() for n in (len(qpos), n_keys + 3, n_keys + 3))
    return q, K, V


def _out(q, K, V, vis, d):
    return _bf(P.reference(q, K, V, d ** -0.5, vis))


def _heads_rejected(kind, name, wrong, ref, base, sees, atol):
    """a wrong output is rejected in every head by a factor >= 2: rule a for the rows that may see the plant, rule c for the others"""
    worst = math.inf
    for h in range(H):
        m = P.measure(wrong[h], ref[h], base[h], sees, atol)
        f = m.leak if kind == "c" else m.err
        assert f >= 2.0, f"{name}, head {h}: the wrong reference is only {f:.2f} x the bound away"
        with pytest.raises(AssertionError):
            P.check(name, wrong[h], ref[h], base[h], sees, atol)
        worst = min(worst, f)
    return worst


def _probe_context(name, seed, d, qpos, n_keys, plants, atol, causal=True, masked_keys=(), vmax=None):
    """one context: the base run, then every plant with its wrong references.  -> (worst honest err / bound, weakest rejection / bound)"""
    qpos_t = torch.tensor(qpos)
    q, K0, V0 = _scene(seed, d, qpos, n_keys)
    N = n_keys + 3
    inside = torch.arange(N)[None, :] < n_keys
    km = torch.ones(N, dtype=torch.int32)
    for jm in masked_keys:
        km[jm] = 0
    vis = (P.causal_visible(qpos_t, N, km) if causal else (km != 0)[None, :].expand(len(qpos), N)) & inside
    base = _out(q, K0, V0, vis, d)
    honest_worst, weakest = 0.0, math.inf
    for j in plants:
        c = P.plant_value(n_keys, vmax)                   # what the GPU tests plant: by the number of keys of the context
        K, V = K0.clone(), V0.clone()
        K[:, j], V[:, j] = 0.0, c
        sees = vis[:, j].clone()
        ref = P.reference(q, K, V, d ** -0.5, vis)
        tag = f"{name} j={j}"
        if not sees.any():                                 # the plant under a zero of the mask: nothing may move
            assert j in masked_keys
            assert torch.equal(_bf(ref), base)               # the honest output is the base run's, bit for bit
            seen = vis.clone()
            seen[:, j] = P.causal_visible(qpos_t, N)[:, j] if causal else True
            weakest = min(weakest, _heads_rejected("c", tag + " masked key seen", _out(q, K, V, seen, d), ref, base, sees, atol))
            continue
        honest = _bf(ref)
        for h in range(H):
            m = P.check(tag, honest[h], ref[h], base[h], sees, atol)
            honest_worst = max(honest_worst, m.err)
        # key j dropped
        dropped = vis.clone()
        dropped[:, j] = False
        weakest = min(weakest, _heads_rejected("a", tag + " dropped", _out(q, K, V, dropped, d), ref, base, sees, atol))
        # key j counted twice (a single visible key has no multiplicity to get wrong: softmax over {j, j} is j)
        if int(vis[sees].sum(dim=1).max()) > 1:
            K2, V2 = torch.cat([K, K[:, j:j + 1]], dim=1), torch.cat([V, V[:, j:j + 1]], dim=1)
            vis2 = torch.cat([vis, vis[:, j:j + 1]], dim=1)
            weakest = min(weakest, _heads_rejected("a", tag + " duplicated", _out(q, K2, V2, vis2, d), ref, base, sees, atol))
        # key j taken from row j + 1 (the stale row when j is the last key)
        Ks, Vs = K.clone(), V.clone()
        Ks[:, j], Vs[:, j] = K[:, j + 1], V[:, j + 1]
        weakest = min(weakest, _heads_rejected("a", tag + " taken from row j + 1", _out(q, Ks, Vs, vis, d), ref, base, sees, atol))
        if causal:
            # the diagonal one key late: the row AT j does not see it
            if (qpos_t == j).any():
                late = vis & P.causal_visible(qpos_t - 1, N)
                weakest = min(weakest, _heads_rejected("a", tag + " diagonal late", _out(q, K, V, late, d), ref, base, sees, atol))
            # the diagonal one key early: the row at j - 1 sees it
            if (qpos_t == j - 1).any():
                early = P.causal_visible(qpos_t + 1, N, km) & inside
                weakest = min(weakest, _heads_rejected("c", tag + " diagonal early", _out(q, K, V, early, d), ref, base, sees, atol))
    if causal:
        # the stale rows past the last position hold K = 0, V = 1e4: an honest kernel gives the base bits, one that sees row pos + 1 does not
        K, V = K0.clone(), V0.clone()
        K[:, n_keys:], V[:, n_keys:] = 0.0, P.STALE_VALUE
        none = torch.zeros(len(qpos), dtype=torch.bool)
        ref = P.reference(q, K, V, d ** -0.5, vis)
        assert torch.equal(_bf(ref), base)
        stale = P.causal_visible(qpos_t + 1, N, km)
        stale[:, :n_keys] = vis[:, :n_keys]
        weakest = min(weakest, _heads_rejected("c", f"{name} stale row seen", _out(q, K, V, stale, d), ref, base, none, atol))
    return honest_worst, weakest


@pytest.mark.parametrize("d,batch_keys,pos,masked,kv8,dtype", P.decode_host_contexts())
def test_probe_rejects_wrong_decode_kernels(d, batch_keys, pos, masked, kv8, dtype):
    """every (head dim, batch size, position, mask, cache format, bound) a case of P.flash_cases() / P.phased_cases() reaches, the positions of the
    per-row launches included (a row of those takes a subset of the position's plants)"""
    mk = P.decode_masked_keys(pos) if masked else ()
    plants = P.decode_plants(pos, batch_keys, masked) + list(mk)
    honest, weakest = _probe_context(f"decode d={d} pos={pos}", 1000 + pos + d, d, [pos], pos + 1, plants, P.atol_of(dtype), masked_keys=mk,
                                     vmax=P.E4M3_MAX if kv8 else None)
    print(f"decode d={d} batch={batch_keys} pos={pos} masked={int(masked)} kv8={int(kv8)} {dtype}: honest {honest:.3f} x bound, "
          f"weakest wrong reference {weakest:.1f} x bound")
    assert honest <= 1.0 and weakest >= 2.0


@pytest.mark.parametrize("R,ctx_max,p,masked,dtype", P.verify_host_contexts())
def test_probe_rejects_wrong_verify_kernels(R, ctx_max, p, masked, dtype):
    mk = P.verify_masked_keys(p) if masked else ()
    plants = P.verify_plants(p, R, P.verify_splits(ctx_max), masked) + list(mk)
    honest, weakest = _probe_context(f"verify p={p} R={R}", 2000 + p + R, 128, list(range(p, p + R)), p + R, plants, P.atol_of(dtype, wide=True),
                                     masked_keys=mk)
    print(f"verify R={R} ctx_max={ctx_max} p={p} masked={int(masked)} {dtype}: honest {honest:.3f} x bound, weakest wrong reference {weakest:.1f} x bound")
    assert honest <= 1.0 and weakest >= 2.0


@pytest.mark.parametrize("T", sorted({c[3] for c in P.CAUSAL_CASES}))
def test_probe_rejects_wrong_causal_prefill_kernels(T):
    plants = P.PREFILL_CAUSAL[T]
    rows = sorted({r for j in plants for r in (j - 1, j, j + 1)} | {0, T - 1})        # the rows around every plant stand for the T rows
    rows = [r for r in rows if 0 <= r < T]
    honest, weakest = _probe_context(f"prefill T={T}", 3000 + T, 128, rows, T, plants, P.ATOL_BF16)
    print(f"causal prefill T={T}: honest {honest:.3f} x bound, weakest wrong reference {weakest:.1f} x bound")
    assert honest <= 1.0 and weakest >= 2.0


@pytest.mark.parametrize("Tq,Tk,wide", sorted({(c[4], c[5], c[1] == 3) for c in P.BIDIR_CASES}))
def test_probe_rejects_wrong_bidirectional_kernels(Tq, Tk, wide):
    rows = sorted({0, 1, 63, 64, 128, 199, Tq - 1})          # a sample of the Tq rows: every row sees every key
    honest, weakest = _probe_context(f"bidirectional {Tq}x{Tk}", 4000 + Tk, 64, rows, Tk, P.PREFILL_BIDIR[Tk], P.atol_of("bf16", wide), causal=False)
    print(f"bidirectional {Tq}x{Tk} wide={int(wide)}: honest {honest:.3f} x bound, weakest wrong reference {weakest:.1f} x bound")
    assert honest <= 1.0 and weakest >= 2.0


def test_plant_value_and_tables():
    assert P.plant_value(1) == 4.0 and P.plant_value(2048) == 512.0 and P.plant_value(2048, P.E4M3_MAX) == 448.0
    assert torch.tensor(P.plant_value(1901)).to(torch.bfloat16).item() == P.plant_value(1901)
    # the batch sizes the issue names: d = 128 bf16, 128 keys at 4 waves and 32 at 2
    assert (P.flash_batch_keys(128, 4), P.flash_batch_keys(128, 2)) == (128, 32)
    assert P.decode_plants(700, 128) == [0, 127, 128, 255, 256, 698, 699, 700]
    assert P.decode_plants(0, 128) == [0] and P.decode_positions(1024)[-1] == 1023
    per = P.verify_split_len(1900, 16, 8)
    assert per == 256 and {per - 1, per, 7 * per - 1, 7 * per} <= set(P.verify_plants(1900, 16, 8))

"""Per-token log-probabilities and scored continuations on the GPU: the stats pass and the pick of
csrc/logprobs.hip through the C ABI against float64 on the host, and generate_many / chat_many with `logprobs` / `target_ids` against the
same calls without them, against the CPU oracle and against forward()."""
import ctypes as C
import dataclasses
import math
import random

import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model
from tests.test_gpu_inflight import BUDGETS, _as_dicts, _cut, _requests

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from visualcla import _lib as L
    return L


# ------------------------------------------------------------------ 1. the stats pass against float64 on the host
SENT_ID, SENT_LP = -77, 123.5
ROW_KINDS = ("ties", "dominant", "constant", "random")


def _row(kind, V, g):
    """fp32 logits with |x| <= 64"""
    if kind == "ties":            # multiples of 0.5: equal values inside the top k and across the k-th place
        return ((torch.randn(V, generator=g) * 2).clamp(-64, 64) * 2).round() / 2
    if kind == "dominant":        # every other exp underflows: lse == max
        x = torch.full((V,), -64.0)
        x[int(torch.randint(0, V, (1,), generator=g))] = 64.0
        return x
    if kind == "constant":        # every logprob is -log V, ids 0 .. k-1
        return torch.full((V,), 3.25)
    return (torch.randn(V, generator=g) * 8).clamp(-64, 64)


def _stats_case(V, B, pad, kind0, seed):
    L = _lib()
    k, cap = min(20, V), 3
    g = torch.Generator().manual_seed(seed)
    kinds = [ROW_KINDS[(b + kind0) % 4] for b in range(B)]
    x = torch.stack([_row(kd, V, g) for kd in kinds])
    if V > k and "ties" in kinds:                                # plant a tie exactly across the k-th place of the first such row
        b = kinds.index("ties")
        order = torch.sort(x[b], descending=True, stable=True).indices
        x[b, order[k - 1:k + 2]] = float(x[b, order[k - 1]])
    ld = V + pad
    buf = torch.full((B, ld), 1e30)                              # a read past V would show: +1e30 wins every maximum
    buf[:, :V] = x
    lens = [int(torch.randint(0, cap, (1,), generator=g)) for _ in range(B)]
    if B >= 3:
        lens[1] = -1                                             # a skipped row
    dev = buf.to(DEV)
    top_ids = torch.full((cap, B, k), SENT_ID, dtype=torch.int64, device=DEV)
    top_lp = torch.full((cap, B, k), SENT_LP, dtype=torch.float32, device=DEV)
    tok_lp = torch.full((cap, B), SENT_LP, dtype=torch.float32, device=DEV)
    lse = torch.full((B,), SENT_LP, dtype=torch.float32, device=DEV)
    copy = torch.full((B, V), SENT_LP, dtype=torch.float32, device=DEV)
    a = L.logprob_args(k, tok_lp, top_ids, top_lp)
    L.logprob_rows(dev[:, :V], torch.tensor(lens, dtype=torch.int32, device=DEV), a, cap, lse=lse, copy=copy)
    top_ids, top_lp, lse, copy = top_ids.cpu(), top_lp.cpu(), lse.cpu(), copy.cpu()
    assert bool((tok_lp == SENT_LP).all())                       # the stats pass does not write the token's own value
    want_lp = torch.log_softmax(x.double(), dim=-1)
    want_lse = torch.logsumexp(x.double(), dim=-1)
    err = 0.0
    for b in range(B):
        if lens[b] < 0:
            assert bool((top_ids[:, b] == SENT_ID).all()) and bool((top_lp[:, b] == SENT_LP).all()) and float(lse[b]) == SENT_LP, (b, "skipped row touched")
            assert bool((copy[b] == SENT_LP).all())
            continue
        order = torch.sort(x[b], descending=True, stable=True).indices[:k]     # equal values: lower id first
        assert torch.equal(top_ids[lens[b], b], order), (kinds[b], b, top_ids[lens[b], b].tolist(), order.tolist())
        err = max(err, float((top_lp[lens[b], b].double() - want_lp[b, order]).abs().max()), abs(float(lse[b]) - float(want_lse[b])))
        assert torch.equal(copy[b], x[b])
        for h in range(cap):
            if h != lens[b]:
                assert bool((top_ids[h, b] == SENT_ID).all()) and bool((top_lp[h, b] == SENT_LP).all())
        if kinds[b] == "dominant":
            assert float(lse[b]) == 64.0 and float(top_lp[lens[b], b, 0]) == 0.0
        if kinds[b] == "constant":
            assert top_ids[lens[b], b].tolist() == list(range(k))
            assert float((top_lp[lens[b], b] + math.log(V)).abs().max()) < 1e-4
    return err


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("V", [5, 1023, 1025, 49958])
def test_logprob_rows_vs_float64(V, B, pad):
    # 1e-4 absolute: ~49 sequential adds per lane plus a 10-level tree over terms <= 1 keep the relative error of the sum below 1e-5, the
    # rounding of x - max at |x| <= 64 is below 1e-5: about 5x of room
    err = max(_stats_case(V, B, pad, kind0, seed=V * 7 + B + pad + kind0) for kind0 in (range(4) if B == 1 else (0, 2)))
    print(f"[logprobs] V={V} B={B} ld=V+{pad}: max |dlogprob| vs float64 = {err:.3e}")
    assert err < 1e-4


def test_logprob_rows_refusals():
    L = _lib()
    x = torch.zeros(2, L.SAMPLE_MAX_VOCAB + 1, device=DEV)
    n = torch.zeros(2, dtype=torch.int32, device=DEV)
    a = L.logprob_args(0, torch.zeros(1, 2, device=DEV))
    with pytest.raises(ValueError, match=str(L.SAMPLE_MAX_VOCAB)):
        L.logprob_rows(x, n, a, 1)
    bad = L.logprob_args(0, torch.zeros(1, 2, device=DEV))
    bad.k = 21
    with pytest.raises(ValueError, match="k=21"):
        L.logprob_rows(x[:, :100], n, bad, 1)


# ------------------------------------------------------------------ 2. the pick
def test_logprob_pick_forced_ids_and_raw_values_behind_the_sampler():
    L = _lib()
    lib = L.load()
    B, V, cap, k = 6, 1025, 5, 8
    g = torch.Generator().manual_seed(3)
    raw = (torch.randn(B, V, generator=g) * 3).clamp(-64, 64)
    raw[0, 700] = 30.0                                           # row 0: the argmax is in the history under repetition_penalty 1.3 and stays the argmax
    raw[1, 9] = 30.0                                             # row 1: the argmax is the eos id, banned by min_new_tokens; the row is FORCED onto it
    raw[2, 11] = 25.0                                            # row 2: forced onto a token of rank 3
    lens = [2, 1, 0, 3, -1, 4]
    hist = torch.randint(20, 600, (cap, B), generator=g)
    hist[0, 0] = 700
    order = torch.sort(raw, dim=-1, descending=True, stable=True).indices
    forced = torch.full((cap, B), -1, dtype=torch.int64)
    forced[1, 1] = 9
    forced[0, 2] = int(order[2, 3])
    forced[0, 4] = 5                                             # an inactive row: never read
    forced[2, 5] = 3                                             # row 5 at another step: not this step's
    kw = dict(repetition_penalty=1.3, min_new_tokens=3, eos_ids=[9], temperature=0.7, top_k=1, top_p=1.0)
    n_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    hist_d = hist.to(DEV)
    # the sampler alone, on its own copy of the raw logits
    plain = torch.full((B,), -9, dtype=torch.int64, device=DEV)
    lg = raw.to(DEV)
    L.check(lib.vcla_sample_rows(lg.data_ptr(), V, B, V, n_dev.data_ptr(), C.byref(L.sample_args(history=hist_d, **kw)), plain.data_ptr(), L.stream_ptr()))
    assert int(plain[0]) == 700 and int(plain[1]) != 9 and float(lg[0, 700]) != 30.0 and float(lg[1, 9]) == float("-inf")
    # stats pass -> sampler on the copy -> pick on the raw rows
    raw_d = raw.to(DEV)
    tok_lp = torch.full((cap, B), SENT_LP, dtype=torch.float32, device=DEV)
    top_ids = torch.full((cap, B, k), SENT_ID, dtype=torch.int64, device=DEV)
    top_lp = torch.full((cap, B, k), SENT_LP, dtype=torch.float32, device=DEV)
    forced_d = forced.to(DEV)                                    # (the struct holds a bare pointer: the tensor must stay alive)
    a = L.logprob_args(k, tok_lp, top_ids, top_lp, forced_d)
    work = torch.empty(B, V, dtype=torch.float32, device=DEV)
    lse = L.logprob_rows(raw_d, n_dev, a, cap, copy=work)
    ids = torch.full((B,), -9, dtype=torch.int64, device=DEV)
    L.check(lib.vcla_sample_rows(work.data_ptr(), V, B, V, n_dev.data_ptr(), C.byref(L.sample_args(history=hist_d, **kw)), ids.data_ptr(), L.stream_ptr()))
    assert torch.equal(ids, plain)                               # the sampler's arithmetic is what it is without logprobs
    assert torch.equal(raw_d.cpu(), raw)                         # and the raw rows are intact
    L.logprob_pick(raw_d, n_dev, a, cap, lse, ids)
    ids, tok_lp, top_ids, top_lp = ids.cpu(), tok_lp.cpu(), top_ids.cpu(), top_lp.cpu()
    want_ids = plain.cpu().clone()
    want_ids[1], want_ids[2] = 9, int(order[2, 3])
    assert torch.equal(ids, want_ids) and int(ids[4]) == -9
    ref = torch.log_softmax(raw.double(), dim=-1)
    for b, h in enumerate(lens):
        col = tok_lp[:, b]
        if h < 0:
            assert bool((col == SENT_LP).all())
            continue
        assert abs(float(col[h]) - float(ref[b, ids[b]])) < 1e-4 and bool((torch.cat([col[:h], col[h + 1:]]) == SENT_LP).all()), b
        rank = (top_ids[h, b] == ids[b]).nonzero()
        if len(rank):                                            # the same value - lse as the stats pass wrote at that rank
            assert float(col[h]) == float(top_lp[h, b, int(rank[0])]), b
    assert int((top_ids[lens[2], 2] == ids[2]).nonzero()[0]) == 3 and int((top_ids[lens[0], 0] == 700).nonzero()[0]) == 0
    assert int((top_ids[lens[1], 1] == 9).nonzero()[0]) == 0     # the banned eos is still the raw distribution's first


# ------------------------------------------------------------------ 3. end to end, fp32, against the same call without logprobs and the oracle
_REF = {}


def _ref(which):
    """(cfg, W, requests, oracle tokens, oracle log_softmax [n_i, V]) of the 12 requests, every one alone -- computed once per model"""
    if which not in _REF:
        cfg = O.cfg_tiny() if which == "tiny" else O.cfg_small()
        W = O.make_weights(cfg, seed=0)
        reqs = _requests(cfg)
        toks, lps = [], []
        for ids, px, n in reqs:
            t, logits = O.visualcla_generate(ids, px, torch.ones_like(ids), W, cfg, max_new_tokens=n, return_logits=True)
            toks.append(t[0])
            lps.append(torch.log_softmax(torch.cat(logits, dim=0).float(), dim=-1))
        _REF[which] = (cfg, W, reqs, toks, lps, make_hip_model(cfg, W, torch.float32))
    return _REF[which]


def _check_shapes(out, k):
    n = out.tokens.numel()
    assert out.tokens.dtype == torch.int64 and out.logprobs.dtype == torch.float32 and out.top_ids.dtype == torch.int64 and out.top_logprobs.dtype == torch.float32
    assert tuple(out.logprobs.shape) == (n,) and tuple(out.top_ids.shape) == (n, k) and tuple(out.top_logprobs.shape) == (n, k)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("which", ["tiny", "small"])
def test_generate_many_logprobs_vs_oracle_fp32(which, share):
    cfg, W, reqs, want, want_lp, m = _ref(which)
    K = 5
    kw = dict(max_batch=4, do_sample=False, eos_token_id=None, share_prefix=share)
    base = m.generate_many(_as_dicts(reqs), steps_per_sync=3, **kw)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(base, want))
    err, compared, pairs = 0.0, 0, 0
    for sps, graph in ((1, True), (3, True), (8, True), (3, False)):
        got = m.generate_many(_as_dicts(reqs), steps_per_sync=sps, use_graph=graph, logprobs=K, **kw)
        st = m.last_inflight_stats
        assert st["logprobs"] == K and st["forced_requests"] == 0 and st["slots"] == 4
        for i, o in enumerate(got):
            _check_shapes(o, K)
            assert torch.equal(o.tokens, base[i]), (sps, graph, i)
            assert torch.equal(o.top_ids[:, 0], o.tokens) and torch.equal(o.top_logprobs[:, 0], o.logprobs), (sps, graph, i)   # plain greedy
            ref = want_lp[i]
            top = torch.sort(ref, dim=-1, descending=True, stable=True)
            err = max(err, float((o.logprobs.cpu() - ref.gather(1, want[i][:, None])[:, 0]).abs().max()),
                      float((o.top_logprobs.cpu() - top.values[:, :K]).abs().max()))
            gap = top.values[:, :K + 1][:, :-1] - top.values[:, 1:K + 1]                 # rank r to rank r + 1
            clear = gap >= 2e-3
            clear[:, 1:] &= gap[:, :-1] >= 2e-3                                         # and rank r - 1 to rank r
            assert torch.equal(o.top_ids.cpu()[clear], top.indices[:, :K][clear]), (sps, graph, i)
            compared += int(clear.sum())
            pairs += clear.numel()
        assert got[0].tokens.numel() == 1 and got[0].logprobs.numel() == 1                # a budget of 1 returns one value
    print(f"[logprobs] {which} share_prefix={share}: max |dlogprob| vs the oracle = {err:.3e}; top ids compared at {compared} of {pairs} (step, rank) pairs")
    assert err < 2e-3                                            # twice the fp32 logit bound 1e-3: a log-probability is a difference of two such quantities
    assert compared >= 0.9 * pairs


def test_generate_many_logprobs_early_eos_and_one_slot():
    cfg, W, reqs, want, want_lp, m = _ref("tiny")
    eos = sorted({int(want[r][len(want[r]) // 2]) for r in (7, 9, 11)})
    full = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=None, logprobs=3)
    got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=eos, logprobs=3)
    n_early = 0
    for i, (o, f) in enumerate(zip(got, full)):
        exp = _cut(want[i], eos)
        n = len(exp)
        n_early += n < len(want[i])
        _check_shapes(o, 3)
        assert torch.equal(o.tokens.cpu(), exp), i
        assert float((o.logprobs - f.logprobs[:n]).abs().max()) < 1e-5 and float((o.top_logprobs - f.top_logprobs[:n]).abs().max()) < 1e-5, i
    assert n_early >= 3
    # a queue of one request, and max_batch = 1, stay on the slots route at one slot (the persistent B = 1 step produces no logits)
    one = m.generate_many(_as_dicts(reqs[9:10]), do_sample=False, eos_token_id=None, logprobs=2)
    assert m.last_inflight_stats["slots"] == 1 and "admission_s" in m.last_inflight_stats
    # (one slot runs other GEMM shapes than four: compared with the oracle, under its bound)
    assert torch.equal(one[0].tokens, full[9].tokens) and float((one[0].logprobs.cpu() - want_lp[9].gather(1, want[9][:, None])[:, 0]).abs().max()) < 2e-3
    two = m.generate_many(_as_dicts(reqs[3:5]), max_batch=1, do_sample=False, eos_token_id=None, logprobs=0)
    assert [torch.equal(a.tokens, b.tokens) for a, b in zip(two, full[3:5])] == [True, True] and tuple(two[1].top_ids.shape) == (BUDGETS[4], 0)
    assert float((two[1].logprobs.cpu() - want_lp[4].gather(1, want[4][:, None])[:, 0]).abs().max()) < 2e-3
    # without the argument the return value is what it was
    plain = m.generate_many(_as_dicts(reqs[3:5]), do_sample=False, eos_token_id=None)
    assert all(isinstance(x, torch.Tensor) for x in plain) and "logprobs" not in m.last_inflight_stats
    with pytest.raises(ValueError, match="request 1: target_ids outside the vocabulary"):
        m.generate_many([_as_dicts(reqs)[1], dict(input_ids=reqs[1][0][0], target_ids=[3, cfg.text.vocab_size])], logprobs=0)


def test_generate_many_logprobs_keep_the_tokens_under_the_sampler_and_mixed_configs():
    cfg, W, reqs, want, want_lp, m = _ref("tiny")
    kw = dict(do_sample=True, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=3, min_new_tokens=4)
    plain = m.generate(input_ids=reqs[11][0].cuda(), max_new_tokens=40, eos_token_id=None, **kw)[0].cpu()
    for eos in (None, int(plain[6])):
        for share in (False, True):
            base = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=2, eos_token_id=eos, share_prefix=share, **kw)
            got = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=2, eos_token_id=eos, share_prefix=share, logprobs=4, **kw)
            for i, (o, b) in enumerate(zip(got, base)):
                assert torch.equal(o.tokens, b), (eos, share, i)
                hit = o.top_ids == o.tokens[:, None]             # RAW scores: where the token is among the top ids, its value is that rank's
                assert torch.equal(o.logprobs[hit.any(dim=1)], o.top_logprobs[hit]), (eos, share, i)
                assert bool((o.logprobs <= o.top_logprobs[:, 0]).all()) and bool(torch.isfinite(o.logprobs).all())
    # the raw distribution does not depend on the config: where sampler and greedy runs took the same tokens, the values are the greedy run's
    greedy = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=None, logprobs=4)
    samp = m.generate_many(_as_dicts(reqs), max_batch=4, eos_token_id=None, logprobs=4, **kw)
    for o, g in zip(samp, greedy):
        same = int((o.tokens == g.tokens).cumprod(0).sum())      # the common prefix
        n = min(same + 1, o.tokens.numel())                      # the distribution of the first differing step is still the same
        assert float((o.top_logprobs[:n] - g.top_logprobs[:n]).abs().max()) < 1e-5
    # two config classes in one queue: per-slot records
    mixed = _as_dicts(reqs)
    for i in range(1, 12, 2):
        mixed[i]["generation_config"] = dict(kw)
    base = m.generate_many(mixed, max_batch=4, do_sample=False, eos_token_id=None)
    got = m.generate_many(mixed, max_batch=4, do_sample=False, eos_token_id=None, logprobs=2)
    assert m.last_inflight_stats["config_classes"] == 2
    for i, (o, b) in enumerate(zip(got, base)):
        assert torch.equal(o.tokens, b), i
        if i % 2 == 0:
            assert torch.equal(o.tokens, greedy[i].tokens) and float((o.logprobs - greedy[i].logprobs).abs().max()) < 1e-5


# ------------------------------------------------------------------ 4. teacher-forced requests
@pytest.mark.parametrize("which", ["tiny", "small"])
def test_generate_many_forced_targets_fp32(which):
    cfg, W, reqs, want, want_lp, m = _ref(which)
    kw = dict(max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=None)
    greedy = m.generate_many(_as_dicts(reqs), logprobs=5, **kw)
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    for i in (4, 9):                                             # an image request and a text one
        a = want[i]
        q = _as_dicts(reqs)
        q[i] = dict(input_ids=reqs[i][0][0], pixel_values=None if reqs[i][1] is None else reqs[i][1][0], target_ids=a)
        got = m.generate_many(q, logprobs=5, **kw)
        assert m.last_inflight_stats["forced_requests"] == 1
        assert torch.equal(got[i].tokens.cpu(), a) and float((got[i].logprobs - greedy[i].logprobs).abs().max()) < 1e-5
        assert float((got[i].top_logprobs - greedy[i].top_logprobs).abs().max()) < 1e-5
        for j in range(12):                                      # the neighbours are not disturbed
            assert torch.equal(got[j].tokens, greedy[j].tokens), (i, j)
        # one token replaced at step 3: the oracle's teacher-forced values on prompt + a'
        a2 = a.clone()
        a2[3] = 3 + (int(a[3]) + 1) % (hi - 3)
        q[i]["target_ids"] = a2.tolist()
        got2 = m.generate_many(q, logprobs=5, **kw)[i]
        ids, px, n = reqs[i]
        full = torch.cat([ids, a2[None, :-1]], dim=1)
        lg = O.visualcla_forward(full, px, torch.ones_like(full), W, cfg)[0, ids.shape[1] - 1:]
        ref = torch.log_softmax(lg.float(), dim=-1)
        assert ref.shape[0] == n and torch.equal(got2.tokens.cpu(), a2)
        err = float((got2.logprobs.cpu() - ref.gather(1, a2[:, None])[:, 0]).abs().max())
        err_top = float((got2.top_logprobs.cpu() - torch.sort(ref, dim=-1, descending=True).values[:, :5]).abs().max())
        print(f"[logprobs] {which} request {i}: forced a' vs the oracle's teacher-forced pass: max |dlogprob| = {err:.3e}, top-5 {err_top:.3e}")
        assert err < 2e-3 and err_top < 2e-3
        assert float((got2.logprobs[:3] - greedy[i].logprobs[:3]).abs().max()) < 1e-5
        assert float((got2.top_logprobs[:4] - greedy[i].top_logprobs[:4]).abs().max()) < 1e-5
        assert int(got2.top_ids[3, 0]) == int(a[3])               # top_* still says what the model would have taken
    # a forced request ends at the first eos of its config, its eos included
    q = [dict(input_ids=reqs[9][0][0], target_ids=want[9]), _as_dicts(reqs)[3]]
    cut = m.generate_many(q, max_batch=4, do_sample=False, eos_token_id=int(want[9][5]), logprobs=1)[0]
    n = int((want[9] == want[9][5]).nonzero()[0]) + 1
    assert torch.equal(cut.tokens.cpu(), want[9][:n]) and cut.logprobs.numel() == n and tuple(cut.top_ids.shape) == (n, 1)
    # a first token that ends the request still returns its one value
    one = m.generate_many([dict(input_ids=reqs[9][0][0], target_ids=[int(want[9][0])]), _as_dicts(reqs)[0]], max_batch=4, do_sample=False, eos_token_id=None, logprobs=1)
    assert one[0].logprobs.numel() == 1 and abs(float(one[0].logprobs[0]) - float(greedy[9].logprobs[0])) < 1e-5 and one[1].logprobs.numel() == 1


def test_generate_many_scores_candidates_behind_one_image():
    cfg, W, reqs, want, want_lp, m = _ref("small")
    ids, px, _ = reqs[4]
    g = torch.Generator().manual_seed(11)
    cands = [torch.randint(3, 200, (n,), generator=g).tolist() for n in (3, 7, 1, 12)]
    q = [dict(input_ids=ids[0], pixel_values=px[0], target_ids=c) for c in cands]
    # a sampling config: forced requests draw nothing and are no sampler rows
    kw = dict(max_batch=4, do_sample=True, top_k=40, temperature=0.7, eos_token_id=None, logprobs=2)
    state = torch.cuda.get_rng_state()
    off = m.generate_many(q, **kw)
    assert m.last_inflight_stats["sampler_rows"] == 0 and m.last_inflight_stats["forced_requests"] == 4
    assert torch.equal(torch.cuda.get_rng_state(), state)        # nothing was taken from the device generator
    on = m.generate_many(q, share_prefix=True, **kw)
    assert m.last_inflight_stats["vision_runs"] == 1 and m.last_inflight_stats["rows_reused"] > 0
    err = 0.0
    for c, a, b in zip(cands, off, on):
        assert a.tokens.tolist() == c == b.tokens.tolist()
        err = max(err, float((a.logprobs - b.logprobs).abs().max()), float((a.top_logprobs - b.top_logprobs).abs().max()))
        full = torch.cat([ids, torch.tensor(c[:-1], dtype=torch.int64)[None]], dim=1)
        ref = torch.log_softmax(O.visualcla_forward(full, px, torch.ones_like(full), W, cfg)[0, ids.shape[1] - 1:].float(), dim=-1)
        assert float((a.logprobs.cpu() - ref.gather(1, torch.tensor(c)[:, None])[:, 0]).abs().max()) < 2e-3
    print(f"[logprobs] 4 candidates behind one image: share_prefix on vs off max |dlogprob| = {err:.3e}")
    assert err < 2e-3
    # the first tokens of all candidates see one distribution
    assert all(float((o.top_logprobs[0] - off[0].top_logprobs[0]).abs().max()) < 1e-5 for o in off)


# ------------------------------------------------------------------ 5. bf16 / W8A16 at the LLaMA-7B widths, rows crossing 512 keys
@pytest.mark.parametrize("fp8", [False, True])
def test_generate_many_logprobs_bf16_engine_widths(fp8):
    """The bound is twice the engine-versus-launch logit bounds of tests/test_gpu_engine.py (0.2 max / 0.04 mean): 0.4 max / 0.08 mean on the
    log-probabilities.  Measured on MI355X (bf16 weights): max 0.0365, mean 0.0094 over 144 steps."""
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=1024))
    m = make_hip_model(cfg, O.make_weights(cfg, seed=2), torch.bfloat16)
    if fp8:
        m.enable_fp8_decode(True, prefill=False)
    g = torch.Generator().manual_seed(1)
    rng = random.Random(4)
    reqs = []
    for r in range(6):
        T = [505, 498, 490][r % 7] if r % 7 < 3 else rng.randint(20, 300)
        reqs.append((torch.randint(3, 4000, (1, T), generator=g), None, rng.randint(18, 40)))
    kw = dict(max_batch=8, steps_per_sync=8, do_sample=False, eos_token_id=None)
    base = m.generate_many(_as_dicts(reqs), **kw)
    got = m.generate_many(_as_dicts(reqs), logprobs=3, **kw)
    assert m.last_inflight_stats["slots"] == 6 or m.last_inflight_stats["slots"] == 8
    assert any(ids.shape[1] < 512 < ids.shape[1] + n for ids, _, n in reqs)
    decode_from = m.last_inflight_stats["decode_from"]
    mx, total, count = 0.0, 0.0, 0
    for (ids, _, n), o, b, p0 in zip(reqs, got, base, decode_from):
        assert torch.equal(o.tokens, b) and torch.equal(o.top_ids[:, 0], o.tokens) and torch.equal(o.top_logprobs[:, 0], o.logprobs)
        if fp8:
            continue                                             # forward() runs the bf16 weights: no reference for the fp8 copies here
        toks = o.tokens.cpu()[None]
        pad = p0 - ids.shape[1]
        full = torch.cat([torch.zeros(1, pad, dtype=torch.int64), ids, toks[:, :-1]], dim=1)
        mask = torch.cat([torch.zeros(1, pad, dtype=torch.int64), torch.ones(1, full.shape[1] - pad, dtype=torch.int64)], dim=1)
        lg = m(input_ids=full.cuda(), attention_mask=mask.cuda()).logits[0].float()
        ref = torch.log_softmax(lg[p0 - 1:p0 - 1 + n], dim=-1).gather(1, o.tokens[:, None])[:, 0]
        d = (o.logprobs - ref).abs()
        mx, total, count = max(mx, float(d.max())), total + float(d.sum()), count + n
    if not fp8:
        print(f"[logprobs] bf16 engine widths: |dlogprob| vs forward() max {mx:.4f} mean {total / count:.4f} over {count} steps")
        assert mx < 0.4 and total / count < 0.08


# ------------------------------------------------------------------ 6. chat_many
from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_many_logprobs(loaded, capsys):  # noqa: F811
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    from visualcla.inflight import RequestOutput
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    gc = GenerationConfig(max_new_tokens=7, do_sample=False, eos_token_id=None)
    img = _image()
    texts = ["what is this?", "hello world", "a cat sitting on a mat", "describe the image"]
    want = visualcla.chat_many(model, [(img, t) for t in texts], generation_config=gc, max_batch=3)
    got = visualcla.chat_many(model, [(img, t) for t in texts], generation_config=gc, max_batch=3, logprobs=3)
    capsys.readouterr()
    assert len(got) == len(want)
    for (r1, h1), (r2, h2, out) in zip(want, got):
        assert r1 == r2 and h1 == h2 and isinstance(out, RequestOutput)
        assert out.tokens.numel() == 7 and tuple(out.logprobs.shape) == (7,) and tuple(out.top_ids.shape) == (7, 3) == tuple(out.top_logprobs.shape)
        assert tokenizer.decode(out.tokens, skip_special_tokens=True) == r2
        assert torch.equal(out.top_ids[:, 0], out.tokens) and bool((out.logprobs <= 0).all())

"""Per-request token constraints decided on the device on the GPU: the mask and the transition of
csrc/constrain.hip through the C ABI against torch.where / a host walk, the device sampler behind the mask against the sampling oracle,
and generate_many / chat_many with `allowed_token_ids` / `banned_token_ids` / `choices` against the CPU oracle, against the same call
without constraints and against generate(prefix_allowed_tokens_fn=...)."""
import ctypes as C
import dataclasses
import random

import numpy as np
import pytest
import torch

from oracle import sampling_oracle as S
from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model
from tests.test_gpu_inflight import BUDGETS, _as_dicts, _requests

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")


def _lib():
    from visualcla import _lib as L
    return L


def _table(node_sets):
    """[(tokens, deny, next or None)] -> (nodes, edges) device tensors; an edge's next is the node itself unless `next` gives one per token"""
    nodes, edges = [], []
    for s, (toks, deny, nxt) in enumerate(node_sets):
        toks = sorted(toks)
        nodes.append([len(edges), len(toks), int(deny), 0])
        edges.extend([t, s if nxt is None else nxt[t]] for t in toks)
    return torch.tensor(nodes, dtype=torch.int32, device=DEV), torch.tensor(edges, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ 1. the mask kernel against torch.where
def _planted_sets(V, g):
    a = sorted({0, V - 1})
    w = sorted({t for t in (31, 32) if t < V} or {V // 2})       # straddling a word where the row has one
    one = [V // 2]
    rnd = torch.randperm(V, generator=g)[:max(1, V // 3)].tolist()
    sets = [a, w, one, list(range(V)), rnd]
    return [(s, False, None) for s in sets] + [(s, True, None) for s in sets]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("V", [5, 33, 1023, 1025, 49958])
def test_constrain_rows_vs_torch_where(V, B, pad):
    L = _lib()
    g = torch.Generator().manual_seed(V * 5 + B + pad)
    sets = _planted_sets(V, g)
    nodes, edges = _table(sets)
    n_nodes = len(sets)
    for off in range(0, n_nodes + B + 1, B):                         # B = 1 and 3 rotate through every node; the last launches carry the skipped rows
        node_of = [(off + b) % n_nodes for b in range(B)]        # B = 64: rows share nodes
        lens = [int(torch.randint(0, 4, (1,), generator=g)) for _ in range(B)]
        state = list(node_of)
        if B == 64:
            state[5], lens[7], state[11], lens[11] = -1, -1, -1, -3
        elif off >= n_nodes:
            state[0] = -1
            if B > 1:
                lens[1] = -1
        elif B == 1 and off == 3:
            lens[0] = -2
        x = torch.randn(B, V, generator=g) * 4
        x[:, 1 % V] = NEG                                        # logits that already hold -inf, kept or not
        x[torch.rand(B, V, generator=g) < 0.05] = NEG
        buf = torch.full((B, V + pad), 1e30)
        buf[:, :V] = x
        dev = buf.to(DEV)
        st = torch.tensor(state, dtype=torch.int32, device=DEV)
        L.constrain_rows(dev[:, :V], torch.tensor(lens, dtype=torch.int32, device=DEV), L.constrain_args(nodes, edges, st))
        got = dev.cpu()
        assert st.tolist() == state                              # the mask does not move the state
        if pad:
            assert bool((got[:, V:] == 1e30).all()), "pad columns touched"
        for b in range(B):
            if state[b] < 0 or lens[b] < 0:
                assert torch.equal(got[b, :V].view(torch.int32), x[b].view(torch.int32)), (off, b, "a skipped row was touched")
                continue
            toks, deny, _ = sets[state[b]]
            keep = torch.zeros(V, dtype=torch.bool)
            keep[toks] = True
            if deny:
                keep = ~keep
            want = torch.where(keep, x[b], torch.full_like(x[b], NEG))
            assert torch.equal(got[b, :V], want), (V, B, pad, off, b, state[b])


def test_constrain_rows_refusals():
    L = _lib()
    nodes, edges = _table([([0], False, None)])
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.constrain_args(nodes, edges, st)
    with pytest.raises(ValueError, match=str(L.CS_MAX_VOCAB)):   # a bitmask beyond 64 KiB of LDS
        L.constrain_rows(torch.zeros(1, L.CS_MAX_VOCAB + 1, device=DEV), n, a)
    bad = L.constrain_args(nodes, edges, st)
    bad.n_nodes = 0
    with pytest.raises(ValueError, match="n_nodes=0"):
        L.constrain_rows(torch.zeros(1, 8, device=DEV), n, bad)
    with pytest.raises(ValueError, match="n_nodes=0"):
        L.constrain_advance(torch.zeros(1, dtype=torch.int64, device=DEV), n, bad)


# ------------------------------------------------------------------ 2. the transition
def test_constrain_advance_hits_misses_deny_and_skipped_rows():
    L = _lib()
    nodes, edges = _table([([3, 10, 20, 50], False, {3: 1, 10: 2, 20: 3, 50: 0}),     # node 0
                           ([5], False, {5: 3}),                                      # node 1: id 0 is no edge
                           ([3, 10], True, {3: 0, 10: 0}),                            # node 2: deny, whatever its edges point to
                           ([0, 7], False, {0: 1, 7: 3})])                            # node 3: id 0 IS an edge
    #        first   last  middle  miss  deny  skipped  0 on an all -inf row  unconstrained  0 that is an edge  a miss above every edge
    state = [0,      0,    0,      0,    2,    0,       1,                    -1,            3,                 0]
    ids = [3,        50,   20,     4,    3,    10,      0,                    3,             0,                 51]
    lens = [0,       0,    1,      2,    0,    -1,      0,                    0,             5,                 0]
    want = [1,       0,    3,      0,    2,    0,       1,                    -1,            1,                 0]
    st = torch.tensor(state, dtype=torch.int32, device=DEV)
    ids_d = torch.tensor(ids, dtype=torch.int64, device=DEV)
    L.constrain_advance(ids_d, torch.tensor(lens, dtype=torch.int32, device=DEV), L.constrain_args(nodes, edges, st))
    assert st.tolist() == want and ids_d.tolist() == ids
    # an all -inf row takes id 0 (the tie rule of vcla_argmax), and the state of a node without that edge does not move
    x = torch.randn(1, 64, device=DEV)
    x[0, 5] = NEG                                                # the only allowed token is banned already: the mask leaves nothing
    st1 = torch.tensor([1], dtype=torch.int32, device=DEV)
    z = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.constrain_args(nodes, edges, st1)
    L.constrain_rows(x, z, a)
    assert bool((x == NEG).all())
    taken = L.argmax(x)
    assert taken.tolist() == [0]
    L.constrain_advance(taken, z, a)
    assert st1.tolist() == [1]


# ------------------------------------------------------------------ 3. the device sampler behind the mask
SAMPLER_CASES = [("allow 4 under top_k 40", [7, 300, 301, 1024], dict(temperature=0.8, top_k=40, top_p=1.0)),
                 ("allow 1", [513], dict(temperature=1.3, top_k=40, top_p=0.9)),
                 ("allowed id in the history under a repetition penalty", [7, 300, 301, 1024], dict(repetition_penalty=1.3, temperature=1.0, top_k=40, top_p=0.95))]


@pytest.mark.parametrize("name,allowed,kw", SAMPLER_CASES, ids=[c[0] for c in SAMPLER_CASES])
def test_sampler_on_the_device_mask_equals_host_mask_and_oracle(name, allowed, kw):
    L = _lib()
    lib = L.load()
    B, V, cap = 8, 1025, 6
    g = torch.Generator().manual_seed(len(name))
    raw = (torch.randn(B, V, generator=g) * 3).clamp(-30, 30)
    lens = [0, 1, 2, 3, 4, 5, 2, 3]
    hist = torch.randint(20, 200, (cap, B), generator=g)
    hist[0, 2:] = allowed[0]                                     # an allowed id in the history of the rows that have one
    hist[1, 4:] = allowed[-1]
    uni = torch.rand(cap, B, generator=g)
    nodes, edges = _table([(allowed, False, None)])
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    n_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    hist_d, uni_d = hist.to(DEV), uni.to(DEV)

    def draw(x):
        ids = torch.full((B,), -9, dtype=torch.int64, device=DEV)
        L.check(lib.vcla_sample_rows(x.data_ptr(), V, B, V, n_dev.data_ptr(), C.byref(L.sample_args(uniforms=uni_d, history=hist_d, **kw)), ids.data_ptr(), L.stream_ptr()))
        return ids.cpu()
    keep = torch.zeros(V, dtype=torch.bool)
    keep[allowed] = True
    host = torch.where(keep[None], raw, torch.full_like(raw, NEG))
    on_dev = raw.to(DEV)
    L.constrain_rows(on_dev, n_dev, L.constrain_args(nodes, edges, st))
    assert torch.equal(on_dev.cpu(), host)
    got, want = draw(on_dev), draw(host.to(DEV))
    assert torch.equal(got, want) and bool(torch.isin(got, torch.tensor(allowed)).all())
    cfg = S.SampleCfg(**kw)
    ref = [int(S.sample_step(host[b:b + 1].numpy(), hist[:lens[b], b:b + 1].numpy(), cfg, np.array([float(uni[lens[b], b])]))[0]) for b in range(B)]
    assert got.tolist() == ref, (name, got.tolist(), ref)
    if len(allowed) > 1:
        assert len(set(got.tolist())) > 1                        # the uniforms do pick different ids


# ------------------------------------------------------------------ 4. end to end, fp32, against the CPU oracle
EOS = 2
_REF = {}


def _spec_queue(cfg, free):
    """the constraints of the 12 requests: unconstrained (0, 4, 9, 11), allow lists, ban lists of what the request would have said, and
    choices -- one a prefix of another, choices sharing a first token, two requests with identical choices, one cut by its budget"""
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    t = lambda k: 3 + (k * 37) % (hi - 3)                        # noqa: E731  (ids below the image tokens)
    A = [[t(1)], [t(1), t(2)], [t(1), t(3), t(4)], [t(5), t(6)]]
    Bc = [[t(7), t(8), t(9)], [t(10)], [t(7), t(11)]]
    Cc = [[t(12), t(13), t(14), t(15)], [t(12), t(16)]]
    ban = lambda i: sorted(set(free[i][:4].tolist()) - {EOS})    # noqa: E731
    return [None, dict(choices=Cc), dict(banned_token_ids=ban(2)), dict(choices=A), None, dict(allowed_token_ids=[t(k) for k in range(20, 26)]),
            dict(choices=[list(c) for c in reversed(A)]), dict(banned_token_ids=ban(7)), dict(choices=Bc), None,
            dict(allowed_token_ids=[t(30), EOS, t(31)]), None]


def _keep(spec, gen, V):
    """the oracle's model of a constraint: bool [V] of what request may take behind the generated ids `gen`"""
    (key, val), = spec.items()
    keep = torch.zeros(V, dtype=torch.bool)
    if key == "allowed_token_ids":
        keep[val] = True
    elif key == "banned_token_ids":
        keep[:] = True
        keep[val] = False
    else:
        n = len(gen)
        nxt = {c[n] for c in val if len(c) > n and list(c[:n]) == gen}
        if any(list(c) == gen for c in val) or not nxt:
            nxt |= {EOS}
        keep[sorted(nxt)] = True
    return keep


def _select(spec, V, margins):
    def fn(logits, generated):
        x = torch.where(_keep(spec, generated[0].tolist(), V)[None], logits, torch.full_like(logits, NEG))
        top2 = x[0].topk(2).values
        if float(top2[1]) > NEG:
            margins.append(float(top2[0] - top2[1]))
        return x.argmax(dim=-1)
    return fn


def _ref(which):
    """(cfg, requests, their constraints, the oracle's tokens of every request alone under its constraint, without it, the model) -- once per model"""
    if which not in _REF:
        cfg = O.cfg_tiny() if which == "tiny" else O.cfg_small()
        W = O.make_weights(cfg, seed=0)
        reqs = _requests(cfg)
        V = cfg.text.vocab_size
        free = [O.visualcla_generate(ids, px, torch.ones_like(ids), W, cfg, max_new_tokens=n, eos_token_id=EOS)[0] for ids, px, n in reqs]
        specs = _spec_queue(cfg, free)
        margins, want = [], []
        for (ids, px, n), sp, f in zip(reqs, specs, free):
            want.append(f if sp is None else O.visualcla_generate(ids, px, torch.ones_like(ids), W, cfg, max_new_tokens=n, eos_token_id=EOS,
                                                                  select_fn=_select(sp, V, margins))[0])
        print(f"[constraints] {which}: smallest top-2 margin among the kept logits over {len(margins)} constrained steps = {min(margins):.3e}")
        assert min(margins) >= 1e-4, "equality of ids is not decidable at this margin: pick other constraint ids"
        _REF[which] = (cfg, W, reqs, specs, want, free, make_hip_model(cfg, W, torch.float32))
    return _REF[which]


def _queue(reqs, specs):
    q = _as_dicts(reqs)
    for r, sp in zip(q, specs):
        if sp is not None:
            r.update(sp)
    return q


def _check_structure(out, spec, eos, budget):
    """what holds under every config: choices spell one choice plus an eos (or its cut), allow lists hold, banned ids never appear"""
    toks = out.tolist()
    (key, val), = spec.items()
    if key == "allowed_token_ids":
        assert set(toks) <= set(val), (toks, val)
    elif key == "banned_token_ids":
        assert not set(toks) & set(val), (toks, val)
    else:
        full = [list(c) + [e] for c in val for e in eos]
        assert any(toks == f[:budget] for f in full) and (len(toks) == budget or toks[-1] in eos), (toks, val)


def test_oracle_outputs_show_the_constraints_at_work():
    cfg, W, reqs, specs, want, free, m = _ref("tiny")
    for i, sp in enumerate(specs):
        if sp is not None:
            _check_structure(want[i], sp, [EOS], BUDGETS[i])
            assert not torch.equal(want[i], free[i]), i          # every constraint changes what its request says
    assert len(want[1]) == 2 and want[1].tolist() == specs[1]["choices"][0][:2]      # the budget cuts the choice


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("which", ["tiny", "small"])
def test_generate_many_constraints_vs_oracle_fp32(which, share, graph):
    cfg, W, reqs, specs, want, free, m = _ref(which)
    kw = dict(max_batch=4, do_sample=False, eos_token_id=EOS, share_prefix=share, use_graph=graph)
    for sps in (1, 3, 8):
        base = m.generate_many(_as_dicts(reqs), steps_per_sync=sps, **kw)
        assert "constrained_requests" not in m.last_inflight_stats
        got = m.generate_many(_queue(reqs, specs), steps_per_sync=sps, **kw)
        st = m.last_inflight_stats
        # A and its reversed copy are one automaton: 7 trie nodes + END; Bc and Cc 6 + END each; two allow and two deny nodes
        assert st["constrained_requests"] == 8 and st["automaton_nodes"] == 8 + 7 + 7 + 4 and st["slots"] == 4
        for i, sp in enumerate(specs):
            if sp is None:
                assert torch.equal(got[i], base[i]) and torch.equal(got[i].cpu(), free[i]), (sps, i)
            else:
                assert torch.equal(got[i].cpu(), want[i]), (sps, i, sp, got[i].tolist(), want[i].tolist())


def test_generate_many_constraint_equals_generate_with_prefix_allowed_tokens_fn():
    cfg, W, reqs, specs, want, free, m = _ref("tiny")
    V = cfg.text.vocab_size
    got = m.generate_many(_queue(reqs, specs), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=EOS)
    for i in (3, 5, 7):                                          # choices, an allow list, a ban list
        ids, px, n = reqs[i]
        fn = lambda batch_id, sent, sp=specs[i]: _keep(sp, sent.tolist(), V).nonzero()[:, 0].tolist()      # noqa: E731
        alone = m.generate(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, do_sample=False, eos_token_id=EOS,
                           prefix_allowed_tokens_fn=fn)[0]
        assert torch.equal(got[i], alone), (i, got[i].tolist(), alone.tolist())


def test_generate_many_one_constrained_request_stays_on_the_slots_route():
    cfg, W, reqs, specs, want, free, m = _ref("tiny")
    for i in (3, 5):
        one = m.generate_many(_queue(reqs[i:i + 1], specs[i:i + 1]), do_sample=False, eos_token_id=EOS)
        assert m.last_inflight_stats["slots"] == 1 and "admission_s" in m.last_inflight_stats and m.last_inflight_stats["constrained_requests"] == 1
        assert torch.equal(one[0].cpu(), want[i]), i
    two = m.generate_many(_queue(reqs[7:9], specs[7:9]), max_batch=1, do_sample=False, eos_token_id=EOS)
    assert [torch.equal(a.cpu(), b) for a, b in zip(two, want[7:9])] == [True, True]
    # refusals that need the resolved config reach the caller by request index, before anything runs
    q = _queue(reqs, specs)
    with pytest.raises(ValueError, match=r"request 1: choices needs an eos_token_id"):
        m.generate_many(q, max_batch=4, do_sample=False, eos_token_id=None)
    with pytest.raises(ValueError, match=rf"request 5: allowed_token_ids outside the vocabulary 0\.\.{cfg.text.vocab_size - 1}"):
        m.generate_many([dict(r, allowed_token_ids=[3, cfg.text.vocab_size]) if i == 5 else r for i, r in enumerate(q)], max_batch=4, do_sample=False, eos_token_id=EOS)


# ------------------------------------------------------------------ 5. other configurations: structure
SAMPLING = dict(do_sample=True, top_k=40, top_p=0.95, temperature=0.9, repetition_penalty=1.1)


def _structure_all(got, specs, eos_of):
    for i, sp in enumerate(specs):
        if sp is not None:
            _check_structure(got[i].cpu(), sp, eos_of(i), BUDGETS[i])


def test_generate_many_constraints_under_a_sampler_mixed_configs_and_seeds():
    cfg, W, reqs, specs, want, free, m = _ref("tiny")
    # a sampling config for the whole queue, two eos ids
    eos2 = [EOS, 5]
    got = m.generate_many(_queue(reqs, specs), max_batch=4, steps_per_sync=3, eos_token_id=eos2, **SAMPLING)
    assert m.last_inflight_stats["sampler_rows"] == 12
    _structure_all(got, specs, lambda i: eos2)
    # two config classes: the odd requests sample under their own eos list, the even ones are greedy under the queue's
    mixed = _queue(reqs, specs)
    for i in range(1, 12, 2):
        mixed[i]["generation_config"] = dict(SAMPLING, eos_token_id=[EOS, 6])
    got = m.generate_many(mixed, max_batch=4, steps_per_sync=2, do_sample=False, eos_token_id=EOS, share_prefix=True)
    assert m.last_inflight_stats["config_classes"] == 2
    _structure_all(got, specs, lambda i: [EOS, 6] if i % 2 else [EOS])
    for i in (6, 8, 10):                                         # the greedy class is still the oracle's
        assert torch.equal(got[i].cpu(), want[i]), i
    # a seeded constrained request gives the same tokens at two queue positions
    seeded = dict(_queue(reqs, specs)[8], seed=1234, generation_config=dict(SAMPLING))
    a = m.generate_many([seeded] + _queue(reqs, specs)[:5], max_batch=4, do_sample=False, eos_token_id=EOS)[0]
    b = m.generate_many(_queue(reqs, specs)[5:] + [seeded], max_batch=3, steps_per_sync=2, do_sample=False, eos_token_id=EOS)[-1]
    assert torch.equal(a, b)
    _check_structure(a.cpu(), specs[8], [EOS], BUDGETS[8])


def test_generate_many_constraints_with_logprobs_stay_raw():
    cfg, W, reqs, specs, want, free, m = _ref("tiny")
    V = cfg.text.vocab_size
    for extra in (dict(do_sample=False), dict(do_sample=True, top_k=1, repetition_penalty=1.1)):     # the argmax path and the sampler path
        kw = dict(max_batch=4, steps_per_sync=3, eos_token_id=EOS, **extra)
        plain = m.generate_many(_queue(reqs, specs), **kw)
        got = m.generate_many(_queue(reqs, specs), logprobs=5, **kw)
        assert m.last_inflight_stats["logprobs"] == 5 and m.last_inflight_stats["constrained_requests"] == 8
        err, outside = 0.0, 0
        for i, ((ids, px, n), sp, o) in enumerate(zip(reqs, specs, got)):
            assert torch.equal(o.tokens, plain[i]), (extra, i)
            if not extra["do_sample"]:
                assert torch.equal(plain[i].cpu(), want[i]), i
            toks = o.tokens.cpu()
            # the oracle's UNCONSTRAINED distribution along the tokens taken
            full = torch.cat([ids, toks[None, :-1]], dim=1)
            ref = torch.log_softmax(O.visualcla_forward(full, px, torch.ones_like(full), W, cfg)[0, ids.shape[1] - 1:].float(), dim=-1)
            err = max(err, float((o.logprobs.cpu() - ref.gather(1, toks[:, None])[:, 0]).abs().max()),
                      float((o.top_logprobs.cpu() - torch.sort(ref, dim=-1, descending=True).values[:, :5]).abs().max()))
            if sp is not None:
                for t in range(len(toks)):
                    keep = _keep(sp, toks[:t].tolist(), V)
                    outside += int((~keep[o.top_ids[t].cpu()]).sum())
        print(f"[constraints] logprobs beside constraints ({extra}): max |dlogprob| vs the oracle's unconstrained log_softmax = {err:.3e}; {outside} top ids are disallowed ones")
        assert err < 2e-3                                        # the bound of section 7h
        assert outside > 0                                       # top_ids are raw: they do name ids the constraint removed


@pytest.mark.parametrize("fp8", [False, True])
def test_generate_many_constraints_bf16_engine_widths(fp8):
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=1024))
    m = make_hip_model(cfg, O.make_weights(cfg, seed=2), torch.bfloat16)
    if fp8:
        m.enable_fp8_decode(True, prefill=False)
    g = torch.Generator().manual_seed(1)
    rng = random.Random(4)
    reqs = [(torch.randint(3, 4000, (1, [505, 498, 60, 200, 33, 120][r]), generator=g), None, rng.randint(6, 12)) for r in range(6)]
    A = [[100], [100, 200], [100, 300, 400], [500, 600]]
    specs = [dict(choices=A), None, dict(allowed_token_ids=[11, 12, 13, 4100]), dict(banned_token_ids=list(range(3, 2000))), dict(choices=A), dict(choices=[[7, 8, 9, 10, 11]])]
    budgets = [n for _, _, n in reqs]
    kw = dict(max_batch=8, steps_per_sync=8, do_sample=False, eos_token_id=EOS)
    base = m.generate_many(_as_dicts(reqs), **kw)
    got = m.generate_many(_queue(reqs, specs), **kw)
    assert m.last_inflight_stats["automaton_nodes"] == 8 + 1 + 1 + 7          # requests 0 and 4 share one automaton
    assert torch.equal(got[1], base[1])
    for i, sp in enumerate(specs):
        if sp is not None:
            (key, val), = sp.items()
            toks = got[i].tolist()
            if key == "choices":
                assert any(toks == (list(c) + [EOS])[:budgets[i]] for c in val), (i, toks)
            elif key == "allowed_token_ids":
                assert set(toks) <= set(val)
            else:
                assert not set(toks) & set(val) and not set(base[i].tolist()) <= set(range(2000, 4200)) | {EOS}      # the ban did bite
    sampled = m.generate_many(_queue(reqs, specs), max_batch=8, eos_token_id=EOS, **SAMPLING)
    assert set(sampled[2].tolist()) <= {11, 12, 13, 4100} and not set(sampled[3].tolist()) & set(range(3, 2000))


# ------------------------------------------------------------------ 6. chat_many
from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_many_constraints(loaded, capsys):  # noqa: F811
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    eos = tokenizer.eos_token_id
    gc = GenerationConfig(max_new_tokens=6, do_sample=False, eos_token_id=eos)
    img = _image()
    texts = ["what is this?", "hello world", "a cat sitting on a mat", "describe the image"]
    items = [(img, t) for t in texts]
    want = visualcla.chat_many(model, [(img, t) for t in texts], generation_config=gc, max_batch=3)
    cons = [None, dict(choices=[[20, 21], [20], [30, 31, 32]]), dict(allowed_token_ids=[40, 41, 42]), dict(banned_token_ids=list(range(3, 100)))]
    got = visualcla.chat_many(model, items, generation_config=gc, max_batch=3, constraints=cons)
    assert model.last_inflight_stats["constrained_requests"] == 3
    requests, gc2 = _chat_requests(model, items, gc, cons)
    toks = model.generate_many(requests, max_batch=3, generation_config=gc2)
    capsys.readouterr()
    assert got[0] == want[0] and len(got) == 4
    assert toks[1].tolist() in ([20, 21, eos], [20, eos], [30, 31, 32, eos])
    assert set(toks[2].tolist()) <= {40, 41, 42} and len(toks[2]) == 6 and not set(toks[3].tolist()) & set(range(3, 100))
    for (resp, hist), t in zip(got, toks):
        assert resp == tokenizer.decode(t, skip_special_tokens=True) and hist[-1] == {"type": "response", "value": resp}
    with pytest.raises(ValueError, match="constraints has 2 entries for 4 items"):
        visualcla.chat_many(model, items, generation_config=gc, constraints=cons[:2])


def _chat_requests(model, items, gc, cons):
    """the requests chat_many builds for `items`, with the constraints as request keys, and the config it resolves"""
    from visualcla import modeling_utils
    out = []
    for (image, text), c in zip(items, cons):
        gc2, enc = modeling_utils._prepare(model, image, text, [], gc)
        out.append(dict(input_ids=enc.input_ids[0], attention_mask=enc.attention_mask[0], pixel_values=enc.pixel_values, **(c or {})))
    return out, gc2

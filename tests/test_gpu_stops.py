"""Stop sequences decided on the device, streamed tokens and cancellation on the GPU: the bookkeeping kernel with a
stop table through the C ABI against the host model and a brute-force tail comparison, and generate_many / chat_many with
`stop_sequences`, `on_tokens` and `stop=` against the same calls without them, cut, and against generate(stopping_criteria=...)."""
import ctypes as C
import dataclasses
import random

import pytest
import torch

from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model
from tests.test_gpu_inflight import _as_dicts, _requests

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 2


def _lib():
    from visualcla import _lib as L
    return L


def _I():
    from visualcla import inflight
    return inflight


# ------------------------------------------------------------------ 1. the kernel through the C ABI
STEPS, CAP, V, D = 20, 24, 97, 64
LONG16 = list(range(10, 26))


def _cases(rng):
    """(name, tokens already in the history, the ids of the next STEPS steps, stop sequences, budget or None, eos list, active)"""
    f = lambda: rng.randint(50, V - 1)                           # noqa: E731  (filler ids no sequence holds)
    fill = lambda s: s + [f() for _ in range(STEPS - len(s))]    # noqa: E731
    never = [[30 + s] * 15 + [31 + s] for s in range(4)]         # four 16-id sequences that never occur
    return [("len 1", [], fill([f(), f(), f(), f(), f(), 9]), [[9]], None, [], True),
            ("len 2 behind a lone first id", [], fill([f(), f(), 9, f(), f(), f(), 9, 10]), [[9, 10]], None, [], True),
            ("len 16 straddling the admission", [10], fill(LONG16[1:]), [LONG16], None, [], True),
            ("self-overlap 7 7 7 8", [], fill([7, 7, 7, 8]), [[7, 7, 8]], None, [], True),
            ("no sequences", [], fill([9, 10, 7, 7, 8]), [], None, [], True),
            ("four sequences, the third hits", [], fill([9, 10, 13, f(), 20, f(), 9, 10, 13, 14]), [[9, 10, 11], [12], [9, 10, 13, 14], [20, 21]], None, [], True),
            ("inactive", [9], [9] * STEPS, [[9]], None, [], False),
            ("stop and budget at one step", [], fill([f(), f(), 9, 10]), [[9, 10]], 4, [], True),
            ("stop and eos at one step", [], fill([f(), 9, 2]), [[9, 2]], None, [2], True),
            ("longer than what was generated", [], fill([9, 10, f(), f(), f(), f(), f(), 5, 9, 10]), [[5, 9, 10]], None, [], True),
            ("budget ends mid-sequence", [], fill([f(), 9, 10, 11]), [[9, 10, 11]], 3, [], True),
            ("eos inside a sequence", [], fill([9, 2, 10]), [[9, 10]], None, [2], True),
            ("two tokens straddling the admission", [9], fill([10]), [[9, 10]], None, [], True),
            ("4 x 16 ids, never a hit", [], fill([30] * 15 + [f()]), never, None, [], True),
            ("two sequences end at one step", [], fill([f(), 3, 4]), [[3, 4], [4]], None, [], True)]


def _expected_end(case):
    """brute force: the count at which the slot finishes (None: it is still active after STEPS steps)"""
    _, h0, stream, seqs, budget, eos, active = case
    if not active:
        return None
    toks = list(h0)
    for t in stream:
        toks.append(t)
        if _I().stop_hit(toks, seqs) or t in eos or (budget is not None and len(toks) >= len(h0) + budget):
            return len(toks)
    return None


def _drive(L, cases, dt, mode):
    """the slots of `cases` stepped STEPS times through one entry (mode: 'stops', 'null' = the stops entry with a null table, 'rows') ->
    per step (state words, history, cur, x bits)"""
    lib = L.load()
    B = len(cases)
    table = torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)
    row_pos = [40 + b if c[6] else -1 for b, c in enumerate(cases)]
    count = [len(c[1]) for c in cases]
    budget = [CAP if c[4] is None else len(c[1]) + c[4] for c in cases]
    hl = [n if p >= 0 else -1 for n, p in zip(count, row_pos)]
    hist = [[-5] * B for _ in range(CAP)]
    for b, c in enumerate(cases):
        for k, t in enumerate(c[1]):
            hist[k][b] = t
    cur = [77] * B
    st = torch.tensor(row_pos + count + hl + budget + [0] * L.SLOT_SUMMARY_WORDS, dtype=torch.int32, device=DEV)
    hist_t = torch.tensor(hist, dtype=torch.int64, device=DEV)
    cur_t = torch.tensor(cur, dtype=torch.int64, device=DEV)
    x = torch.zeros(B, D, dtype=dt, device=DEV)
    eos_rows = L.slot_eos_rows([c[5] for c in cases]).to(DEV)
    stop_t = L.slot_stop_rows([c[3] for c in cases]).to(DEV)
    sa = L.stop_args(stop_t)
    a = L.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist_t, cur_t, st[4 * B:])
    host = dict(row_pos=row_pos, count=count, budget=budget, hl=hl, hist=hist, cur=cur)
    snaps = []
    for step in range(STEPS):
        ids = [c[2][step] for c in cases]
        ids_t = torch.tensor(ids, dtype=torch.int64, device=DEV)
        if mode == "rows":
            L.check(lib.vcla_slot_step_rows(ids_t.data_ptr(), C.byref(a), eos_rows.data_ptr(), table.data_ptr(), x.data_ptr(), D, V, L.dtype_code(dt), L.stream_ptr()))
        else:
            L.check(lib.vcla_slot_step_stops(ids_t.data_ptr(), C.byref(a), eos_rows.data_ptr(), C.byref(sa) if mode == "stops" else None, table.data_ptr(),
                                             x.data_ptr(), D, V, L.dtype_code(dt), L.stream_ptr()))
        snaps.append((st.tolist(), hist_t.tolist(), cur_t.tolist(), x.cpu().view(torch.int16 if dt == torch.bfloat16 else torch.int32).clone(), ids))
        assert torch.equal(x.float(), table[cur_t].float()), step
    return snaps, host, stop_t


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_slot_step_stops_kernel_vs_host_model_and_brute_force(B, dt):
    I, L = _I(), _lib()
    all_cases = _cases(random.Random(B))
    n = len(all_cases)
    rounds = [[all_cases[(r * B + b) % n] for b in range(B)] for r in range((n + B - 1) // B)]
    seen_end = {}
    for cases in rounds:
        snaps, h, stop_t = _drive(L, cases, dt, "stops")
        for step, (s, hist_d, cur_d, _, ids) in enumerate(snaps):
            n_act = I.slot_step_model(ids, h["row_pos"], h["count"], h["budget"], h["hist"], h["cur"], [], h["hl"], eos_rows=[c[5] for c in cases],
                                      stops=[c[3] for c in cases])
            assert s[:B] == h["row_pos"] and s[B:2 * B] == h["count"] and s[2 * B:3 * B] == h["hl"] and s[3 * B:4 * B] == h["budget"], (step, s[:B], h["row_pos"])
            assert s[4 * B] == n_act and s[4 * B + 1] == 0 and hist_d == h["hist"] and cur_d == h["cur"], step
        assert torch.equal(stop_t.cpu(), L.slot_stop_rows([c[3] for c in cases]))      # the table is read only
        for b, c in enumerate(cases):
            end = _expected_end(c)
            assert (h["count"][b] if h["row_pos"][b] < 0 and c[6] else None) == end, (c[0], h["count"][b], end)
            if not c[6]:                                         # the inactive slot: nothing of it moved
                assert h["count"][b] == len(c[1]) and h["cur"][b] == 77 and all(h["hist"][k][b] == -5 for k in range(len(c[1]), CAP))
            seen_end[c[0]] = end
    assert len(seen_end) == n
    assert seen_end["len 1"] == 6 and seen_end["len 2 behind a lone first id"] == 8 and seen_end["len 16 straddling the admission"] == 16
    assert seen_end["self-overlap 7 7 7 8"] == 4 and seen_end["no sequences"] is None and seen_end["four sequences, the third hits"] == 10
    assert seen_end["stop and budget at one step"] == 4 and seen_end["stop and eos at one step"] == 3 and seen_end["longer than what was generated"] == 10
    assert seen_end["budget ends mid-sequence"] == 3 and seen_end["eos inside a sequence"] == 2 and seen_end["two tokens straddling the admission"] == 2
    assert seen_end["4 x 16 ids, never a hit"] is None and seen_end["two sequences end at one step"] == 3


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_null_stop_table_is_bitwise_slot_step_rows(B, dt):
    L = _lib()
    all_cases = _cases(random.Random(B))
    cases = [all_cases[(b * 5 + 1) % len(all_cases)] for b in range(B)]
    null, _, _ = _drive(L, cases, dt, "null")
    rows, _, _ = _drive(L, cases, dt, "rows")
    for step, (a, b) in enumerate(zip(null, rows)):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3]), step


def test_a_stop_block_without_a_table_is_refused():
    L = _lib()
    B = 2
    st = torch.tensor([-1] * B + [0] * B + [-1] * B + [4] * B + [0] * L.SLOT_SUMMARY_WORDS, dtype=torch.int32, device=DEV)
    hist, cur = torch.zeros(4, B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    a = L.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
    table, x = torch.zeros(V, D, dtype=torch.bfloat16, device=DEV), torch.zeros(B, D, device=DEV)
    bad = L.StopArgs()
    with pytest.raises((ValueError, L.VclaError), match="null stop table"):
        L.check(L.load().vcla_slot_step_stops(cur.data_ptr(), C.byref(a), None, C.byref(bad), table.data_ptr(), x.data_ptr(), D, V, L.dtype_code(torch.float32), L.stream_ptr()))
    with pytest.raises(ValueError, match="contiguous int32"):
        L.stop_args(torch.zeros(B, 4, 8, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ 2. end to end, fp32
_REF = {}


def _ref():
    """(cfg, requests, the model, the free run of the queue under eos 2) -- once"""
    if not _REF:
        cfg = O.cfg_tiny()
        W = O.make_weights(cfg, seed=0)
        reqs = _requests(cfg)
        m = make_hip_model(cfg, W, torch.float32)
        base = [x.cpu().tolist() for x in m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=EOS)]
        assert "stop_requests" in m.last_inflight_stats and m.last_inflight_stats["stop_requests"] == 0
        _REF["x"] = (cfg, reqs, m, base)
    return _REF["x"]


def _stops_from(base):
    """every request's stop sequences taken FROM its own free run, so hits are certain and their places known"""
    stops = [None] * len(base)
    stops[4] = [base[4][5:7]]                                    # two tokens in the middle
    stops[6] = [base[6][:1]]                                     # the first token alone: ends in admission
    stops[8] = [base[8][0:2]]                                    # straddling the admission and the first step
    stops[10] = [[base[10][3], base[10][3], base[10][1], base[10][7]]] if len(set(base[10])) > 3 else [[1, 1]]      # absent
    stops[9] = [base[9][10:26]]                                  # 16 ids
    stops[11] = [[1, 1, 1], base[11][20:23], base[11][30:31] + [1], base[11][33:35]]      # four, the second hits first
    stops[5] = [base[5][-2:] + [1]]                              # its budget ends inside the sequence: no match
    return stops


def _queue(reqs, stops, **extra):
    q = _as_dicts(reqs)
    for r, s in zip(q, stops):
        if s is not None:
            r["stop_sequences"] = s
        r.update(extra)
    return q


def _cut_all(base, stops):
    return [_I().cut_at_stop(b, s) for b, s in zip(base, stops)]


def test_the_free_run_makes_the_stops_bite():
    cfg, reqs, m, base = _ref()
    stops = _stops_from(base)
    want = _cut_all(base, stops)
    assert all(len(base[i]) >= n for i, n in ((4, 7), (8, 2), (9, 26), (11, 35)))
    assert len(want[4]) <= 7 < len(base[4]) and len(want[6]) == 1 and len(want[8]) == 2 and want[10] == base[10] and want[5] == base[5]
    assert len(want[9]) <= 26 < len(base[9]) and len(want[11]) <= 23 < len(base[11])
    assert not _I().stop_hit(base[10], stops[10])


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("share", [False, True])
def test_generate_many_stop_sequences_equal_the_cut_free_run(share, graph):
    cfg, reqs, m, base = _ref()
    stops = _stops_from(base)
    want = _cut_all(base, stops)
    for sps in (1, 3, 8):
        got = m.generate_many(_queue(reqs, stops), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=EOS, share_prefix=share, use_graph=graph)
        st = m.last_inflight_stats
        for i in range(12):
            assert got[i].tolist() == want[i], (share, graph, sps, i, got[i].tolist(), want[i])
        assert st["stop_requests"] == 7 and st["stop_hits"] == sum(_I().stop_hit(w, s) for w, s in zip(want, stops)) >= 5 and st["cancelled"] == 0
        assert st["tokens"] == sum(len(w) for w in want)


def test_stop_sequences_with_logprobs_cut_the_arrays_alike():
    cfg, reqs, m, base = _ref()
    stops = _stops_from(base)
    want = _cut_all(base, stops)
    kw = dict(max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=EOS, logprobs=2)
    free = m.generate_many(_as_dicts(reqs), **kw)
    got = m.generate_many(_queue(reqs, stops), **kw)
    for i in range(12):
        n = len(want[i])
        assert got[i].tokens.tolist() == want[i] and free[i].tokens.tolist() == base[i], i
        assert tuple(got[i].top_ids.shape) == (n, 2) and tuple(got[i].logprobs.shape) == (n,) and tuple(got[i].top_logprobs.shape) == (n, 2)
        # the same fp32 rows under another admission schedule: equal up to the rounding of sums taken in another order
        assert torch.allclose(got[i].logprobs, free[i].logprobs[:n], atol=1e-4, rtol=0) and torch.allclose(got[i].top_logprobs, free[i].top_logprobs[:n], atol=1e-4, rtol=0)
        assert got[i].top_ids[:, 0].tolist() == want[i]


def test_stop_sequences_beside_a_choices_constraint_and_min_new_tokens():
    cfg, reqs, m, base = _ref()
    hi = min(cfg.img_start_token_id, cfg.img_end_token_id, cfg.img_token_id)
    t = lambda k: 3 + (k * 37) % (hi - 3)                        # noqa: E731
    q = _as_dicts(reqs)
    q[3]["choices"] = [[t(1), t(2), t(3), t(4)]]
    kw = dict(max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=EOS)
    free = m.generate_many(q, **kw)
    assert free[3].tolist() == [t(1), t(2), t(3), t(4), EOS]
    q[3]["stop_sequences"] = [[t(2), t(3)]]
    q[7]["stop_sequences"] = [base[7][2:4]]
    got = m.generate_many(q, **kw)
    assert got[3].tolist() == [t(1), t(2), t(3)] and got[7].tolist() == _I().cut_at_stop(base[7], [base[7][2:4]])
    assert m.last_inflight_stats["constrained_requests"] == 1 and m.last_inflight_stats["stop_requests"] == 2
    # min_new_tokens does not delay a stop (HF's floor only suppresses the eos)
    floor = dict(max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=EOS, min_new_tokens=6)
    free6 = [x.tolist() for x in m.generate_many(_as_dicts(reqs), **floor)]
    stops = [None] * 12
    stops[7] = [free6[7][1:3]]
    got6 = m.generate_many(_queue(reqs, stops), **floor)
    assert got6[7].tolist() == _I().cut_at_stop(free6[7], stops[7]) and len(got6[7]) <= 3


def test_stop_sequences_under_seeded_sampling():
    cfg, reqs, m, base = _ref()
    kw = dict(max_batch=4, steps_per_sync=3, do_sample=True, top_k=40, top_p=0.95, temperature=0.9, eos_token_id=EOS)
    seeds = [dict(seed=100 + i) for i in range(12)]
    q = _as_dicts(reqs)
    for r, s in zip(q, seeds):
        r.update(s)
    free = [x.tolist() for x in m.generate_many(q, **kw)]
    stops = [None] * 12
    for i in (4, 7, 9, 11):
        stops[i] = [free[i][3:5]] if len(free[i]) >= 6 else None
    assert sum(s is not None for s in stops) >= 2
    q2 = _queue(reqs, stops)
    for r, s in zip(q2, seeds):
        r.update(s)
    got = m.generate_many(q2, **kw)
    assert [g.tolist() for g in got] == _cut_all(free, stops)


def test_stop_sequences_equal_generate_with_a_stopping_criterion():
    cfg, reqs, m, base = _ref()
    stops = _stops_from(base)
    got = m.generate_many(_queue(reqs, stops), max_batch=4, steps_per_sync=3, do_sample=False, eos_token_id=EOS)
    for i, (ids, px, n) in enumerate(reqs):
        crit = (lambda gen, scores, s=stops[i]: _I().stop_hit(gen[0].tolist(), s)) if stops[i] is not None else None
        alone = m.generate(input_ids=ids.cuda(), pixel_values=None if px is None else px.cuda(), max_new_tokens=n, do_sample=False, eos_token_id=EOS,
                           stopping_criteria=[crit] if crit is not None else None)[0]
        assert got[i].tolist() == alone.tolist(), (i, got[i].tolist(), alone.tolist())


def test_one_request_with_stops_or_a_callback_stays_on_the_slots_route():
    cfg, reqs, m, base = _ref()
    one = m.generate_many(_queue(reqs[4:5], [[base[4][5:7]]]), do_sample=False, eos_token_id=EOS)
    assert m.last_inflight_stats["slots"] == 1 and "admission_s" in m.last_inflight_stats and one[0].tolist() == _I().cut_at_stop(base[4], [base[4][5:7]])
    calls = []
    two = m.generate_many(_as_dicts(reqs[4:6]), max_batch=1, steps_per_sync=4, do_sample=False, eos_token_id=EOS, on_tokens=lambda i, t, f: calls.append((i, t, f)))
    assert "admission_s" in m.last_inflight_stats and [x.tolist() for x in two] == base[4:6]
    assert [i for i, _, _ in calls] == sorted(i for i, _, _ in calls) and m.last_inflight_stats["stream_calls"] == len(calls)
    with pytest.raises(ValueError, match=r"request 1: 5 stop sequences.*request 2: stop sequence 0 holds ids outside the vocabulary"):
        m.generate_many(_queue(reqs[:3], [None, [[5]] * 5, [[cfg.text.vocab_size]]]), do_sample=False, eos_token_id=EOS)
    with pytest.raises(ValueError, match="on_tokens must be a callable"):
        m.generate_many(_as_dicts(reqs[:3]), do_sample=False, on_tokens=3)


# ------------------------------------------------------------------ 3. streaming and cancel
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("sps", [1, 3, 8])
def test_streamed_chunks_concatenate_and_cancel_returns_what_was_delivered(sps, share):
    cfg, reqs, m, base = _ref()
    stops = _stops_from(base)
    want = _cut_all(base, stops)
    calls = []
    got = m.generate_many(_queue(reqs, stops), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=EOS, share_prefix=share,
                          on_tokens=lambda i, t, f: calls.append((i, list(t), f)))
    assert m.last_inflight_stats["stream_calls"] == len(calls) and m.last_inflight_stats["cancelled"] == 0
    for i in range(12):
        mine = [(t, f) for j, t, f in calls if j == i]
        assert got[i].tolist() == want[i] == [x for t, _ in mine for x in t], i
        assert [f for _, f in mine] == [False] * (len(mine) - 1) + [True] and all(1 <= len(t) <= sps + 1 for t, _ in mine), i
    assert [t for j, t, f in calls if j == 0] == [want[0]] and [t for j, t, f in calls if j == 6] == [want[6]]      # ended by their first token: one call
    # cancel request 2 at its second call (and request 9 at its first): exactly the tokens delivered; the others are untouched
    seen, n_calls = {}, {}

    def fn(i, toks, fin):
        seen.setdefault(i, []).extend(toks)
        n_calls[i] = n_calls.get(i, 0) + 1
        return (i == 2 and n_calls[i] == 2) or i == 9
    got2 = m.generate_many(_as_dicts(reqs), max_batch=4, steps_per_sync=sps, do_sample=False, eos_token_id=EOS, share_prefix=share, on_tokens=fn, logprobs=0)
    n2, n9 = min(len(base[2]), 1 + 2 * sps), min(len(base[9]), 1 + sps)
    assert got2[2].tokens.tolist() == seen[2] == base[2][:n2] and got2[9].tokens.tolist() == seen[9] == base[9][:n9]
    assert len(got2[2].logprobs) == n2 and len(got2[9].logprobs) == n9
    assert m.last_inflight_stats["cancelled"] == (n2 < len(base[2])) + (n9 < len(base[9])) >= 1
    for i in range(12):
        if i not in (2, 9):
            assert got2[i].tokens.tolist() == seen[i] == base[i], i


def test_callback_exception_propagates_and_the_model_keeps_working():
    cfg, reqs, m, base = _ref()

    def fn(i, toks, fin):
        raise KeyError("mine")
    with pytest.raises(KeyError, match="mine"):
        m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=EOS, on_tokens=fn)
    again = m.generate_many(_as_dicts(reqs), max_batch=4, do_sample=False, eos_token_id=EOS)
    assert [x.tolist() for x in again] == base


# ------------------------------------------------------------------ 4. bf16 at the engine widths: every request in a slot of its own
def test_stop_sequences_bf16_engine_widths_exact_when_the_schedule_cannot_change():
    cfg = cfg_engine_small()
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, max_position_embeddings=1024))
    m = make_hip_model(cfg, O.make_weights(cfg, seed=2), torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    reqs = [(torch.randint(3, 4000, (1, [505, 498, 60, 200, 33, 120][r]), generator=g), None, [12, 20, 9, 16, 24, 10][r]) for r in range(6)]
    kw = dict(max_batch=8, steps_per_sync=8, do_sample=False, eos_token_id=None)
    base = [x.tolist() for x in m.generate_many(_as_dicts(reqs), **kw)]
    stops = [[base[0][5:7]], [base[1][:1]], None, [base[3][0:2], [1, 1]], [base[4][4:20]], [[1, 1, 1]]]
    got = m.generate_many(_queue(reqs, stops), **kw)
    want = _cut_all(base, stops)
    assert [x.tolist() for x in got] == want and sum(len(a) < len(b) for a, b in zip(want, base)) == 4
    assert m.last_inflight_stats["slots"] == 6 and m.last_inflight_stats["stop_hits"] == 4


# ------------------------------------------------------------------ 5. chat_many
from tests.test_gpu_dropin import loaded  # noqa: E402,F401  (the merged on-disk checkpoint + tokenizer + image processor fixture)


def test_chat_many_stop_strings(loaded, capsys):  # noqa: F811
    from transformers import GenerationConfig
    from tests.test_gpu_dropin import _image
    visualcla, model, tokenizer, image_processor, cfg, W = loaded
    gc = GenerationConfig(max_new_tokens=12, do_sample=False, eos_token_id=None)
    img = _image()
    texts = ["what is this?", "hello world", "a cat sitting on a mat", "describe the image"]
    base = visualcla.chat_many(model, [(img, t) for t in texts], generation_config=gc, max_batch=3)
    k = max(range(len(texts)), key=lambda j: len(base[j][0]))
    full = base[k][0]
    assert len(full) >= 4
    s = full[len(full) // 2:len(full) // 2 + 2]
    seen = []
    got = visualcla.chat_many(model, [(img, t) for t in texts], generation_config=gc, max_batch=3, stops=[[s] if j == k else None for j in range(len(texts))],
                              on_text=lambda i, t, f: seen.append((i, t, f)))
    capsys.readouterr()
    assert got[k][0] == full[:full.find(s)] and got[k][1][-1] == {"type": "response", "value": got[k][0]}
    for j in range(len(texts)):
        if j != k:
            assert got[j][0] == base[j][0], j
        mine = [(t, f) for i, t, f in seen if i == j]
        assert mine[-1] == (got[j][0], True) and all(not f for _, f in mine[:-1]), j
    everyone = visualcla.chat_many(model, [(img, t) for t in texts], generation_config=gc, max_batch=3, stop=[s])
    for j in range(len(texts)):
        assert everyone[j][0] == (base[j][0][:base[j][0].find(s)] if s in base[j][0] else base[j][0]), j

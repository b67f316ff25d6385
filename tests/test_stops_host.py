"""Stop sequences, streamed tokens and cancellation in generate_many / chat_many, host side: the host model of the
bookkeeping kernel against a brute-force tail comparison, the scheduler driven by `simulate` with stops and a cancelling callback, the
refusals by request index, the ABI of the new entries, and chat_many's string logic over a stub tokenizer.  No GPU."""
import os
import random
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vcla_slot_step_stops", "vcla_llama_decode_slots_stops")


def _I():
    from visualcla import inflight
    return inflight


# ------------------------------------------------------------------ 1. the host model of the kernel against a brute-force tail comparison
def _run_stream(stream, seqs, budget=10 ** 6, cap=None, eos=()):
    """one slot fed `stream` through slot_step_model from count 0 -> the number of tokens after which it finished (None: still active)"""
    I = _I()
    cap = len(stream) if cap is None else cap
    row_pos, count, bud, cur, hl = [5], [0], [budget], [0], [0]
    history = [[-3] for _ in range(cap)]
    for n, t in enumerate(stream, 1):
        act = I.slot_step_model([t], row_pos, count, bud, history, cur, list(eos), hl, stops=[seqs])
        assert count[0] == n and cur[0] == t and history[n - 1][0] == t
        if row_pos[0] < 0:
            assert act == 0 and hl[0] == -1
            return n
        assert act == 1 and hl[0] == n and row_pos[0] == 5 + n
    return None


def _brute(stream, seqs, budget=10 ** 6, eos=()):
    for n in range(1, len(stream) + 1):
        tail_hit = any(len(q) and n >= len(q) and stream[n - len(q):n] == list(q) for q in seqs)
        if tail_hit or n >= budget or stream[n - 1] in eos:
            return n
    return None


def test_slot_step_model_stops_vs_brute_force_planted_cases():
    assert _run_stream([7, 7, 7, 8, 1, 2], [[7, 7, 8]]) == 4                       # self-overlapping: the match starts inside a failed one
    assert _run_stream([1, 2, 3, 4, 9], [[3, 4], [2, 3, 4]]) == 4                   # two sequences end at one step
    long16 = list(range(20, 36))
    assert _run_stream([5, 6] + long16 + [1], [long16]) == 18                       # a sequence of the full 16 ids
    assert _run_stream(long16[1:] + [3], [long16]) is None                          # ... whose first id is missing
    assert _run_stream([4, 5], [[3, 4, 5]]) is None                                 # longer than what was generated: no match
    assert _run_stream([4, 5], [[3, 4, 5], [5]]) == 2
    assert _run_stream([9], [[9]]) == 1                                             # the very first token
    assert _run_stream([1, 2, 3], [[1, 2, 3, 4]], budget=3) == 3                    # a budget that ends mid-sequence: the budget ends it
    assert _run_stream([1, 2, 3, 4], [[3, 4]], eos=[3]) == 3                        # the eos comes first
    assert _run_stream([1, 2, 3, 4], [[1, 2]], eos=[4]) == 2                        # the stop comes first
    assert _run_stream([1, 2, 3], []) is None and _run_stream([1, 2, 3], [[]]) is None


def test_slot_step_model_stops_vs_brute_force_random_streams():
    rng = random.Random(7)
    n_hit = n_free = 0
    for case in range(600):
        alphabet = rng.choice([2, 3, 6])
        stream = [rng.randrange(alphabet) for _ in range(rng.randint(1, 40))]
        seqs = [[rng.randrange(alphabet) for _ in range(rng.choice([1, 2, 3, 5, 16]))] for _ in range(rng.randint(0, 4))]
        budget = rng.choice([10 ** 6, rng.randint(1, 40)])
        eos = rng.choice([(), (alphabet - 1,)])
        got, want = _run_stream(stream, seqs, budget, eos=eos), _brute(stream, seqs, budget, eos)
        assert got == want, (case, stream, seqs, budget, eos)
        n_hit += want is not None
        n_free += want is None
    assert n_hit > 100 and n_free > 20


def test_slot_step_model_without_stops_is_unchanged_and_other_slots_are_left_alone():
    I = _I()
    row_pos, count, bud, cur, hl = [3, -1, 8], [2, 4, 1], [9, 9, 9], [0, 77, 0], [2, -1, 1]
    history = [[11, 5, 6], [12, 5, 0], [0, 5, 0], [0, 5, 0], [0, 0, 0]]
    stops = [[[12, 40]], [[5], [77]], []]                           # slot 0 hits across the history, slot 1 is inactive, slot 2 has none
    n = I.slot_step_model([40, 5, 6], row_pos, count, bud, history, cur, [], hl, stops=stops)
    assert n == 1 and row_pos == [-1, -1, 9] and count == [3, 4, 2] and hl == [-1, -1, 2] and cur == [40, 77, 6]
    assert history[2] == [40, 5, 0] and history[1] == [12, 5, 6]


# ------------------------------------------------------------------ 2. the scheduler under `simulate`
BUDGETS = [1, 2, 5, 9, 14, 20, 26, 31, 35, 38, 40, 40, 3, 17, 8, 22]


def _tok(i, k):                                                  # small alphabet: sequences recur inside a stream
    return 10 + (i * 7 + k * k + k // 3) % 5


def _free(i):
    return [_tok(i, k) for k in range(1, BUDGETS[i] + 1)]


def _stops_of(rng):
    out = []
    for i, n in enumerate(BUDGETS):
        f, kind = _free(i), i % 4
        if kind == 0 or n < 3:
            out.append(None if i % 8 else [[999]])               # none / one that never appears
        elif kind == 1:
            out.append([f[:1]])                                  # the first token alone
        elif kind == 2:
            out.append([f[0:2], [998, 997]])                     # straddling admission and the first step
        else:
            p = rng.randint(1, n - 2)
            out.append([f[p:p + 2], f[p:p + 1] + [996]])
    return out


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("sps", [1, 3, 8])
@pytest.mark.parametrize("slots", [1, 4, 16])
def test_simulate_with_stops_every_result_is_the_cut_of_its_free_run(slots, sps, share):
    I = _I()
    stops = _stops_of(random.Random(slots * 10 + sps))
    calls = []
    sch, log = I.simulate(BUDGETS, slots, sps, stops=stops, token_of=_tok, share_prefix=share, on_tokens=lambda i, t, f: calls.append((i, list(t), f)))
    res = sch.ordered_results()
    want = [I.cut_at_stop(_free(i), stops[i]) for i in range(len(BUDGETS))]
    assert res == want
    assert sum(len(a) < len(b) for a, b in zip(want, map(_free, range(len(BUDGETS))))) >= 5
    assert sch.stats["stop_requests"] == sum(s is not None for s in stops) and sch.stats["cancelled"] == 0
    assert sch.stats["stop_hits"] == sum(I.stop_hit(w, s) for w, s in zip(want, stops)) >= 6
    assert sch.stats["stream_calls"] == len(calls)
    _check_calls(calls, res, sps)
    # without stops the same queue runs to its budgets, and takes more steps
    free_sch, _ = I.simulate(BUDGETS, slots, sps, token_of=_tok, share_prefix=share)
    assert free_sch.ordered_results() == [_free(i) for i in range(len(BUDGETS))] and free_sch.stats["steps"] >= sch.stats["steps"]
    assert free_sch.stats["stop_requests"] == free_sch.stats["stop_hits"] == free_sch.stats["stream_calls"] == 0


def _check_calls(calls, results, sps):
    """chunks concatenate to the result, one finished=True call per request and it is the last, no chunk above sps + 1 tokens"""
    for i, want in enumerate(results):
        mine = [(t, f) for j, t, f in calls if j == i]
        assert [x for t, _ in mine for x in t] == want, i
        assert [f for _, f in mine] == [False] * (len(mine) - 1) + [True], i
        assert all(1 <= len(t) <= sps + 1 for t, _ in mine), i


def test_simulate_calls_come_in_ascending_request_order_within_a_boundary():
    I = _I()
    marks = []

    def fn(i, toks, fin):
        marks.append(i)
    sch, log = I.simulate(BUDGETS, 4, 3, token_of=_tok, on_tokens=fn)
    # a boundary's calls ascend; a new boundary starts where the index falls
    runs, cur = [], []
    for i in marks:
        if cur and i <= cur[-1]:
            runs.append(cur)
            cur = []
        cur.append(i)
    runs.append(cur)
    assert all(r == sorted(r) for r in runs) and len(runs) <= sch.stats["steps"] // 3 + 1
    assert sorted(set(marks)) == list(range(len(BUDGETS)))


@pytest.mark.parametrize("sps", [1, 3, 8])
def test_simulate_cancel_frees_the_slot_at_that_boundary_and_returns_what_was_delivered(sps):
    I = _I()
    seen, n_calls = {}, {}
    cancel_at = {5: 2, 9: 1, 11: 3}                              # request -> the call that returns True

    def fn(i, toks, fin):
        seen.setdefault(i, []).extend(toks)
        n_calls[i] = n_calls.get(i, 0) + 1
        return n_calls[i] == cancel_at.get(i)
    calls = []
    sch, log = I.simulate(BUDGETS, 4, sps, token_of=_tok, on_tokens=lambda i, t, f: (calls.append((i, list(t), f)), fn(i, t, f))[1])
    res = sch.ordered_results()
    for i in range(len(BUDGETS)):
        assert res[i] == seen[i] == _free(i)[:len(res[i])], i
        if i not in cancel_at:
            assert res[i] == _free(i), i
    for i, k in cancel_at.items():
        assert len(res[i]) == min(BUDGETS[i], 1 + k * sps) and n_calls[i] == k, (i, res[i])
    n_cancelled = sum(len(res[i]) < BUDGETS[i] for i in cancel_at)
    assert sch.stats["cancelled"] == n_cancelled >= 2
    # the freed slot is refilled at that boundary: the request admitted into request 5's slot arrives at the boundary of 5's cancelling call
    adm = {i: (bd, b) for bd, b, i in log}
    slot5, bd5 = adm[5][1], adm[5][0]
    nxt = min((bd, i) for i, (bd, b) in adm.items() if b == slot5 and bd > bd5)
    assert nxt[0] == bd5 + cancel_at[5], (adm[5], nxt)
    # a cancel is not a finished=True call: the cancelled request's last call has finished=False
    for i in cancel_at:
        if len(res[i]) < BUDGETS[i]:
            assert [f for j, _, f in calls if j == i][-1] is False


def test_simulate_with_logprobs_cancel_keeps_the_arrays_of_the_delivered_tokens():
    I = _I()
    sch, _ = I.simulate([9, 9, 9], 2, 2, logprobs=2, token_of=_tok, on_tokens=lambda i, t, f: i == 1)
    out = sch.ordered_results()
    assert len(out[1].tokens) == 3 and len(out[1].logprobs) == 3 and len(out[1].top_ids) == 3 and len(out[0].tokens) == 9


def test_callback_exception_propagates():
    I = _I()

    def fn(i, toks, fin):
        raise KeyError("mine")
    with pytest.raises(KeyError, match="mine"):
        I.simulate(BUDGETS, 4, 3, token_of=_tok, on_tokens=fn)


# ------------------------------------------------------------------ 3. refusals
def _bare_model():
    from visualcla.modeling_visualcla import VisualCLAModel
    m = VisualCLAModel.__new__(VisualCLAModel)
    m._device = torch.device("cpu")
    m.generation_config = None
    m._ctx = None
    return m


def test_stop_sequences_refusals_name_the_request_in_one_message():
    I = _I()
    m = _bare_model()
    ids = torch.arange(3, 9)
    V = 100
    raw = [dict(input_ids=ids), dict(input_ids=ids, stop_sequences=[[4]] * 5), dict(input_ids=ids, stop_sequences=[[4], []]),
           dict(input_ids=ids, stop_sequences=[list(range(17))]), dict(input_ids=ids, stop_sequences=[[4, 2.5]]),
           dict(input_ids=ids, stop_sequences=[[4, V]]), dict(input_ids=ids, stop_sequences=[[-1]]),
           dict(input_ids=ids, stop_sequences=[[4, 5]], target_ids=[7, 8]), dict(input_ids=ids, stop_sequences=[[True]]),
           dict(input_ids=ids, stop_sequences=[4, 5]), dict(input_ids=ids, stop_sequences=[list(range(16))] * 4)]
    reqs = [m._inflight_request(i, r, 0) for i, r in enumerate(raw)]
    with pytest.raises(ValueError) as e:
        I.check_stop_sequences([r["stops"] for r in reqs], V, [r["target"] is not None for r in reqs])
    msg = str(e.value)
    for want in (r"request 1: 5 stop sequences \(at most 4\)", r"request 2: stop sequence 1 is empty", r"request 3: stop sequence 0 holds 17 ids \(at most 16\)",
                 r"request 4: stop sequence 0 holds non-integers", r"request 5: stop sequence 0 holds ids outside the vocabulary 0\.\.99",
                 r"request 6: stop sequence 0 holds ids outside the vocabulary", r"request 7: stop_sequences beside target_ids",
                 r"request 8: stop sequence 0 holds non-integers", r"request 9: stop_sequences must be a list of lists"):
        assert re.search(want, msg), (want, msg)
    assert "request 0" not in msg and "request 10" not in msg
    # accepted: lists, tuples, tensors; the full 4 x 16
    ok = I.check_stop_sequences([None, [(4, 5)], [torch.tensor([6, 7])], [list(range(16))] * 4], V)
    assert ok[:3] == [None, [[4, 5]], [[6, 7]]] and len(ok[3]) == 4
    # the unknown-keys check knows the new key and nothing else new
    assert m._inflight_request(0, dict(input_ids=ids, stop_sequences=[[4]]))["stops"] == [[4]]
    with pytest.raises(ValueError, match=r"request 0: unknown keys \['stop'\]"):
        m._inflight_request(0, dict(input_ids=ids, stop=[[4]]))


def test_slot_stop_rows_layout_and_checks():
    from visualcla import _lib as L
    t = L.slot_stop_rows([None, [[5]], [[1, 2, 3], list(range(16))]])
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 4, 16)
    assert bool((t[0] == -1).all()) and t[1, 0].tolist() == [5] + [-1] * 15 and bool((t[1, 1:] == -1).all())
    assert t[2, 0].tolist() == [1, 2, 3] + [-1] * 13 and t[2, 1].tolist() == list(range(16))
    for bad in ([[[1]] * 5], [[[]]], [[list(range(17))]], [[[-2]]]):
        with pytest.raises(ValueError, match="slot 0"):
            L.slot_stop_rows(bad)


# ------------------------------------------------------------------ 4. the ABI
def test_new_symbols_are_declared_exported_and_bound():
    from visualcla import _lib as L
    header = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    assert re.search(r"#define\s+VCLA_ABI_VERSION\s+5\b", header)
    for name, val in (("VCLA_SLOT_MAX_STOPS", L.SLOT_MAX_STOPS), ("VCLA_SLOT_MAX_STOP_LEN", L.SLOT_MAX_STOP_LEN)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)\b", header).group(1)) == val, name
    assert (L.SLOT_MAX_STOPS, L.SLOT_MAX_STOP_LEN) == (4, 16) == (_I().SLOT_MAX_STOPS, _I().SLOT_MAX_STOP_LEN)
    assert re.search(r"typedef\s+struct\s+vcla_stop_args\s*\{\s*const\s+int32_t\s*\*\s*seqs\s*;", header)
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1], name
    assert len(L.SYMBOLS["vcla_llama_decode_slots_stops"][1]) == len(L.SYMBOLS["vcla_llama_decode_slots_constrained"][1]) + 1
    assert len(L.SYMBOLS["vcla_slot_step_stops"][1]) == len(L.SYMBOLS["vcla_slot_step_rows"][1]) + 1
    assert lib.vcla_version() == 5


# ------------------------------------------------------------------ 5. chat_many's string logic over a stub tokenizer
class _Tok:
    """id k decodes to WORDS[k]; ids 0..2 are special"""
    WORDS = ["<unk>", "<s>", "</s>", "Hello", " world", "\n", "###", " End", "!", " more"]

    def decode(self, ids, skip_special_tokens=False):
        return "".join(self.WORDS[int(i)] for i in ids if not (skip_special_tokens and int(i) < 3))


def test_text_stops_earliest_string_final_chunk_and_per_item_lists():
    from visualcla.modeling_utils import TextStops
    texts = []
    ts = TextStops(_Tok(), 3, stop=["###", " End"], stops=[None, ["!"], None], on_text=lambda i, t, f: texts.append((i, t, f)))
    assert ts.active and ts.strings_of == [["###", " End"], ["###", " End", "!"], ["###", " End"]]
    # item 0: " End" occurs before "###" in the text although it is listed second: the earliest occurrence wins
    assert ts.on_tokens(0, [3, 4], False) is False
    assert ts.on_tokens(0, [7, 5, 6, 9], False) is True
    assert ts.cut(0, _Tok().decode(ts.tokens[0], True)) == "Hello world"
    # item 1: its own "!" first; the string becomes visible only in the final chunk
    assert ts.on_tokens(1, [3, 1, 4], False) is False
    assert ts.on_tokens(1, [9, 8, 2], True) is True
    assert ts.cut(1, "Hello world more!") == "Hello world more"
    # item 2: a string split over two tokens of two chunks ("\n" then "###" for the stop "\n###")
    ts2 = TextStops(_Tok(), 1, stops=[["\n###"]])
    assert ts2.on_tokens(0, [3, 5], False) is False and ts2.on_tokens(0, [6, 9], False) is True and ts2.cut(0, "Hello\n### more") == "Hello"
    assert ts.on_tokens(2, [3, 9, 2], True) is False and ts.cut(2, "Hello more") == "Hello more"
    assert texts == [(0, "Hello world", False), (0, "Hello world", True), (1, "Hello world", False), (1, "Hello world more", True), (2, "Hello more", True)]
    assert not TextStops(_Tok(), 2).active and TextStops(_Tok(), 2, stop="###").strings_of == [["###"], ["###"]]
    with pytest.raises(ValueError, match="stops has 1 entries for 2 items"):
        TextStops(_Tok(), 2, stops=[None])
    with pytest.raises(ValueError, match="item 1: stop strings must be non-empty str"):
        TextStops(_Tok(), 2, stops=[None, [""]])
    with pytest.raises(ValueError, match="item 0: stop strings"):
        TextStops(_Tok(), 1, stop=[[5, 6]])


def test_chat_many_stop_goes_through_generate_many_on_tokens():
    """chat_many with a stub model: the strings reach generate_many as an on_tokens callback, never as stop_sequences, and the response
    and the history hold the text before the earliest occurrence"""
    from visualcla import modeling_utils as U

    class _Enc(dict):
        __getattr__ = dict.__getitem__

        def to(self, *_):
            return self

    class _Model:
        tokenizer, dtype, device, num_patch = _Tok(), torch.float32, "cpu", 1
        streams = [[3, 4, 5, 6, 9, 9, 2], [3, 9, 8, 9, 2], [3, 4, 2]]

        def generate_many(self, requests, on_tokens=None, **kw):
            assert all("stop_sequences" not in r for r in requests)
            self.kw, outs = kw, []
            for i, s in enumerate(self.streams):                 # boundaries of 3 tokens, as the slots loop delivers them
                got = []
                for k in range(0, len(s), 3):
                    got += s[k:k + 3]
                    if on_tokens is not None and on_tokens(i, s[k:k + 3], k + 3 >= len(s)) and k + 3 < len(s):
                        break
                outs.append(torch.tensor(got))
            return outs
    m = _Model()
    real = U._prepare
    U._prepare = lambda model, image, text, history, gc: (history.append({"type": "instruction", "value": text}), (gc, _Enc(input_ids=torch.zeros(1, 2), attention_mask=torch.ones(1, 2), pixel_values=None)))[1]
    try:
        seen = []
        out = U.chat_many(m, [(None, "a"), (None, "b"), (None, "c")], stop=["\n###"], stops=[None, ["!"], None], on_text=lambda i, t, f: seen.append((i, t, f)))
        plain = U.chat_many(m, [(None, "a"), (None, "b"), (None, "c")])
    finally:
        U._prepare = real
    assert [r for r, _ in out] == ["Hello world", "Hello more", "Hello world"]
    assert [r for r, _ in plain] == ["Hello world\n### more more", "Hello more! more", "Hello world"]
    assert all(h[-1] == {"type": "response", "value": r} for r, h in out)
    assert seen == [(0, "Hello world\n", False), (0, "Hello world", True), (1, "Hello more", True), (2, "Hello world", True)]

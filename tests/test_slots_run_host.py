"""generate_many's run object (visualcla/slots_run.py), host side: cut_calls and start_slots against straight transcriptions of the loop
and of the two admission tails they replace (the in-class methods _inflight_admit_ragged / _inflight_admit before the move).  No GPU."""
import random

import pytest
import torch

from visualcla import _lib
from visualcla.slots_run import Logprobs, PerRequest, SlotsRun, cut_calls

MAX_ROWS, ALONE_ABOVE = 8192, 2048


# ------------------------------------------------------------------ 1. cut_calls
def _loop_before_the_move(rows_of, members, max_rows, alone_above):
    calls, cur_call, m = [], [], 0
    for i in members:
        r = rows_of[i]
        alone = r > alone_above
        if cur_call and (alone or m + r > max_rows):
            calls.append(cur_call)
            cur_call, m = [], 0
        cur_call.append(i)
        m += r
        if alone:
            calls.append(cur_call)
            cur_call, m = [], 0
    if cur_call:
        calls.append(cur_call)
    return calls


@pytest.mark.parametrize("rows, want", [
    ([], []),                                                                    # empty members
    ([100, 2000, 7], [[0, 1, 2]]),                                               # all rows fit in one call
    ([2048, 2048, 2048, 2048, 1], [[0, 1, 2, 3], [4]]),                          # a sum that lands exactly on max_rows
    ([2049, 10, 20], [[0], [1, 2]]),                                             # one member above alone_above: first,
    ([10, 2049, 20], [[0], [1], [2]]),                                           # in the middle,
    ([10, 20, 2049], [[0, 1], [2]]),                                             # last
    ([10, 3000, 2049, 20], [[0], [1], [2], [3]]),                                # two such members adjacent
    ([9000], [[0]]),                                                             # a single member above max_rows is a call of its own
])
def test_cut_calls_hand_cases(rows, want):
    members = list(range(len(rows)))
    assert cut_calls(rows, members, MAX_ROWS, ALONE_ABOVE) == want == _loop_before_the_move(rows, members, MAX_ROWS, ALONE_ABOVE)


def test_cut_calls_random_cases():
    rng = random.Random(0)
    for _ in range(200):
        n = rng.randint(0, 24)
        rows_of = {i: rng.randint(1, 3000) for i in rng.sample(range(100), n)}      # by request index, as the admission passes it
        members = list(rows_of)
        rng.shuffle(members)
        calls = cut_calls(rows_of, members, MAX_ROWS, ALONE_ABOVE)
        assert calls == _loop_before_the_move(rows_of, members, MAX_ROWS, ALONE_ABOVE)
        assert [i for c in calls for i in c] == members and all(calls)
        assert all(len(c) == 1 or sum(rows_of[i] for i in c) <= MAX_ROWS for c in calls)


# ------------------------------------------------------------------ 2. start_slots
B, CAP, W = 4, 6, _lib.SLOT_SUMMARY_WORDS
DEV = torch.device("cpu")


class _Sched:
    """what start_slots touches of an InflightScheduler: the slot count, the budgets, started()"""

    def __init__(self, budget):
        self.slots, self.budget, self.calls = B, budget, []

    def started(self, b, first_token, ended, extra=None):
        self.calls.append((b, first_token, ended, extra))


def _buffers():
    """the slot table as a run starts it; cur and hist hold values no case writes, so a stray write shows"""
    st = torch.tensor([-1] * B + [0] * B + [-1] * B + [0] * B + [0] * W, dtype=torch.int32)
    return st, torch.full((B,), -7, dtype=torch.int64), -torch.arange(1, CAP * B + 1, dtype=torch.int64).view(CAP, B), [0] * B


def _padded_tail_before_the_move(g_requests, g_slots, first_h, Tg, eos, per, lp, sched, st, cur, hist, count_h):
    dev = DEV
    live = []
    for j, (i, b) in enumerate(zip(g_requests, g_slots)):
        ended = first_h[j] in (eos if per is None else per["eos_of"][i]) or sched.budget[i] == 1
        sched.started(b, first_h[j], ended, lp["first"].pop(i) if lp is not None else None)
        if not ended:
            live.append((b, first_h[j], sched.budget[i]))
    if live:
        lb = torch.tensor([x[0] for x in live], device=dev)
        fi = torch.tensor([x[1] for x in live], dtype=torch.int64, device=dev)
        st[lb] = Tg                                         # row_pos
        st[B + lb] = 1                                      # count
        st[2 * B + lb] = 1                                  # hist_len
        st[3 * B + lb] = torch.tensor([x[2] for x in live], dtype=torch.int32, device=dev)
        cur[lb] = fi
        hist[0, lb] = fi
        for b, _, _ in live:
            count_h[b] = 1


def _ragged_tail_before_the_move(g_requests, g_slots, first_of, plan_T, eos, per, lp, sched, st, cur, hist, count_h):
    dev = DEV
    live = []
    for i, b in zip(g_requests, g_slots):
        ended = first_of[i] in (eos if per is None else per["eos_of"][i]) or sched.budget[i] == 1
        sched.started(b, first_of[i], ended, lp["first"].pop(i) if lp is not None else None)
        if not ended:
            live.append((b, first_of[i], sched.budget[i], plan_T[i]))
    if live:
        lb = torch.tensor([x[0] for x in live], device=dev)
        fi = torch.tensor([x[1] for x in live], dtype=torch.int64, device=dev)
        st[lb] = torch.tensor([x[3] for x in live], dtype=torch.int32, device=dev)        # row_pos: every slot decodes from its own T
        st[B + lb] = 1                                      # count
        st[2 * B + lb] = 1                                  # hist_len
        st[3 * B + lb] = torch.tensor([x[2] for x in live], dtype=torch.int32, device=dev)
        cur[lb] = fi
        hist[0, lb] = fi
        for b, _, _, _ in live:
            count_h[b] = 1


def _extras(requests):
    return {i: ([-0.5 - i], [[i, i + 1]], [[-0.5 - i, -2.0]]) for i in requests}


# name: requests, slots, first tokens, budget of every request of the queue, eos of the queue, per-request eos lists, logprobs
CASES = {
    "one_live": ([2], [1], [11], [3, 3, 5], [9], None, False),
    "first_token_is_eos": ([0, 1], [0, 3], [9, 4], [5, 5], [4, 8], None, False),
    "budget_of_one": ([0, 1, 2], [2, 0, 3], [11, 12, 13], [3, 1, 6], [], None, False),
    "per_request_eos": ([0, 1, 2], [3, 1, 0], [6, 6, 5], [4, 4, 4], [], [[5], [6, 7], []], False),
    "logprobs_first": ([1, 3], [0, 2], [7, 9], [2, 2, 2, 2], [9], None, True),
    "per_request_eos_with_logprobs": ([3, 0, 1, 2], [0, 1, 2, 3], [5, 5, 5, 5], [1, 2, 3, 4], [], [[5], [], [5, 6], [4]], True),
    "nobody_lives": ([0, 1], [1, 2], [9, 3], [4, 1], [9], None, False),
}
PLAN_T = [17, 5, 40, 23]                                    # ragged path: the prompt length of every request of the queue
TG = 31                                                     # padded path: the group's length


@pytest.mark.parametrize("ragged", [False, True], ids=["padded_constant", "ragged_table"])
@pytest.mark.parametrize("case", list(CASES))
def test_start_slots_writes_what_the_two_tails_wrote(case, ragged):
    requests, slots, first, budget, eos, eos_of, logprobs = CASES[case]
    # expected: the block of the admission path before the move, on buffers of its own
    want_sched, (st, cur, hist, count_h) = _Sched(budget), _buffers()
    per = dict(eos_of=eos_of) if eos_of is not None else None
    lp = dict(first=_extras(requests)) if logprobs else None
    if ragged:
        _ragged_tail_before_the_move(requests, slots, dict(zip(requests, first)), PLAN_T, eos, per, lp, want_sched, st, cur, hist, count_h)
    else:
        _padded_tail_before_the_move(requests, slots, first, TG, eos, per, lp, want_sched, st, cur, hist, count_h)
    # the run object, on CPU tensors and nothing else
    run = SlotsRun.__new__(SlotsRun)
    run.sched, run.dev, run.eos = _Sched(budget), DEV, eos
    run.st, run.cur, run.hist, run.count_h = _buffers()
    run.per = PerRequest(eos_of, [], None, None, []) if eos_of is not None else None
    run.lp = Logprobs(2, None, None, None, None, None) if logprobs else None
    if logprobs:
        run.lp.first.update(_extras(requests))
    run.start_slots(requests, slots, first, PLAN_T if ragged else TG)
    assert run.sched.calls == want_sched.calls and len(run.sched.calls) == len(requests)
    assert torch.equal(run.st, st) and run.st.dtype == torch.int32
    assert torch.equal(run.cur, cur) and torch.equal(run.hist, hist)
    assert run.count_h == count_h
    if logprobs:
        assert run.lp.first == {} == lp["first"]             # popped per request
    live = [b for b, (_, _, ended, _) in zip(slots, run.sched.calls) if not ended]
    assert run.st[:B].tolist() == [(PLAN_T[requests[slots.index(b)]] if ragged else TG) if b in live else -1 for b in range(B)]
    assert case == "nobody_lives" or live                      # every other case does write

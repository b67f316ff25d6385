"""Per-token log-probabilities and scored continuations in generate_many, host side: argument validation before
any device call, the ABI of the new entries, the scheduler with forced budgets.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from visualcla import inflight as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vcla_logprob_rows", "vcla_logprob_pick", "vcla_llama_decode_slots_logprobs")


def _bare_model():
    """a VisualCLAModel without weights or device: what the argument checks touch"""
    from visualcla.modeling_visualcla import VisualCLAModel
    m = VisualCLAModel.__new__(VisualCLAModel)
    m._device = torch.device("cpu")
    m.generation_config = None
    m._ctx = None
    return m


# ------------------------------------------------------------------ 1. arguments
@pytest.mark.parametrize("bad", [True, -1, 21, 1.5])
def test_logprobs_argument_is_refused_by_name_before_anything_runs(bad):
    from visualcla import modeling_utils
    m = _bare_model()                                            # no config, no context: any step past the check would fail otherwise
    with pytest.raises(ValueError, match="logprobs"):
        m.generate_many([dict(input_ids=torch.arange(3, 9))], logprobs=bad)
    with pytest.raises(ValueError, match="logprobs"):
        modeling_utils.chat_many(None, [], logprobs=bad)
    with pytest.raises(ValueError, match="logprobs"):
        I.check_logprobs(bad)


def test_logprobs_argument_accepts_none_and_the_range():
    assert I.check_logprobs(None) is None
    assert [I.check_logprobs(k) for k in (0, 1, 20)] == [0, 1, 20]
    assert I.RequestOutput._fields == ("tokens", "logprobs", "top_ids", "top_logprobs")


def test_target_ids_request_key():
    m = _bare_model()
    ids = torch.arange(3, 9)
    with pytest.raises(ValueError, match=r"request 3: target_ids needs .*logprobs"):
        m._inflight_request(3, dict(input_ids=ids, target_ids=[4, 5]))
    with pytest.raises(ValueError, match="request 2: target_ids must be a 1-D sequence of at least one"):
        m._inflight_request(2, dict(input_ids=ids, target_ids=[]), 0)
    with pytest.raises(ValueError, match="request 2: target_ids must be"):
        m._inflight_request(2, dict(input_ids=ids, target_ids=[[4, 5]]), 0)
    with pytest.raises(ValueError, match="request 2: target_ids must be"):
        m._inflight_request(2, dict(input_ids=ids, target_ids=[1.5]), 0)
    with pytest.raises(ValueError, match="request 5: target_ids and max_new_tokens"):
        m._inflight_request(5, dict(input_ids=ids, target_ids=[4, 5], max_new_tokens=2), 3)
    r = m._inflight_request(0, dict(input_ids=ids, target_ids=torch.tensor([7, 8, 9])), 0)
    assert r["target"] == [7, 8, 9] and r["max_new_tokens"] is None
    assert m._inflight_request(0, dict(input_ids=ids), 5)["target"] is None
    # the budget of a forced request is the target length, whatever the configs say
    from transformers import GenerationConfig
    assert m._request_budgets(GenerationConfig(max_new_tokens=11), [r], [None], [6]) == [3]


# ------------------------------------------------------------------ 2. the ABI
def test_new_symbols_are_declared_exported_and_bound():
    from visualcla import _lib as L
    header = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    assert re.search(r"#define\s+VCLA_ABI_VERSION\s+5\b", header)
    assert re.search(r"#define\s+VCLA_LOGPROB_MAX_K\s+20\b", header) and L.LOGPROB_MAX_K == 20 == I.LOGPROB_MAX_K
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1], name
    # the new entry is the old one plus one pointer
    assert len(L.SYMBOLS["vcla_llama_decode_slots_logprobs"][1]) == len(L.SYMBOLS["vcla_llama_decode_slots_rows"][1]) + 1
    assert lib.vcla_logprob_scratch_bytes(64, 49958, 1) >= 64 * 49958 * 4 + 64 * 4
    assert lib.vcla_logprob_scratch_bytes(64, 49958, 0) < 4096


def test_logprob_args_size_matches_c(tmp_path):
    from visualcla import _lib as L
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "visualcla_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(vcla_logprob_args), offsetof(vcla_logprob_args, k), offsetof(vcla_logprob_args, token_logprob), "
                   "offsetof(vcla_logprob_args, top_ids), offsetof(vcla_logprob_args, top_logprobs), offsetof(vcla_logprob_args, forced)); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = L.LogprobArgs
    assert got == [C.sizeof(A), A.k.offset, A.token_logprob.offset, A.top_ids.offset, A.top_logprobs.offset, A.forced.offset]


def test_logprob_args_helper_checks_its_buffers():
    from visualcla import _lib as L
    lp = torch.zeros(4, 2)
    with pytest.raises(ValueError, match="logprobs=21"):
        L.logprob_args(21, lp)
    with pytest.raises(ValueError, match="needs top_ids"):
        L.logprob_args(3, lp)
    with pytest.raises(ValueError, match="top_ids must be"):
        L.logprob_args(3, lp, torch.zeros(4, 2, 3), torch.zeros(4, 2, 3))
    a = L.logprob_args(0, lp)
    assert a.k == 0 and a.token_logprob == lp.data_ptr() and not a.top_ids and not a.forced


# ------------------------------------------------------------------ 3. the scheduler with forced budgets
@pytest.mark.parametrize("slots,sps,share", [(1, 1, False), (3, 2, False), (4, 8, True)])
def test_scheduler_returns_per_request_arrays_in_request_order(slots, sps, share):
    budgets = [1, 6, 3, 9, 2, 5, 7]
    targets = [None, [11, 12, 13, 14], None, [21], None, [31, 0, 33], None]      # request 5's target holds the eos id 0 at its 2nd token
    K = 2
    sch, log = I.simulate(budgets, slots, sps, eos_at={6: 3}, share_prefix=share, logprobs=K, targets=targets)
    assert sch.budget == [1, 4, 3, 1, 2, 3, 7]                   # the budget of a forced request is its target length
    out = sch.ordered_results()
    want_tokens = [[1001], [11, 12, 13, 14], [3001, 3002, 3003], [21], [5001, 5002], [31, 0], [7001, 7002, 0]]
    assert [o.tokens for o in out] == want_tokens
    for i, o in enumerate(out):
        n = len(o.tokens)
        assert isinstance(o, I.RequestOutput)
        assert o.logprobs == [-(i + t / 1000) for t in range(n)]
        assert o.top_ids == [[t * 10 + r for r in range(K)] for t in range(n)] and o.top_logprobs == [[-float(i + r) for r in range(K)]] * n
    assert sorted(i for _, _, i in log) == list(range(7)) and sch.stats["tokens"] == sum(len(t) for t in want_tokens)
    # without logprobs the scheduler returns what it always did, and targets are refused
    plain, _ = I.simulate(budgets, slots, sps, eos_at={6: 3}, share_prefix=share)
    assert plain.ordered_results()[2] == [3001, 3002, 3003] and plain.logprobs is None
    with pytest.raises(ValueError, match="targets need logprobs"):
        I.InflightScheduler([4] * 2, [3, 3], [False] * 2, 2, 64, targets=[None, [1]])


def test_scheduler_refuses_a_target_that_does_not_fit_and_a_finish_without_arrays():
    with pytest.raises(ValueError, match="request 1: target_ids of 5 tokens"):
        I.InflightScheduler([4, 60], [3, 3], [False] * 2, 2, 64, logprobs=0, targets=[None, [1] * 5])
    sch = I.InflightScheduler([4], [1], [False], 1, 64, logprobs=1)
    sch.admit(sch.free_slots())
    with pytest.raises(ValueError, match="without one log-probability per token"):
        sch.started(0, 7, True)
    sch.started(0, 7, True, ([-0.5], [[7]], [[-0.5]]))
    assert sch.ordered_results() == [I.RequestOutput([7], [-0.5], [[7]], [[-0.5]])]

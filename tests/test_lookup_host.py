"""Prompt-lookup decoding, host side: the package's restatement of draft selection (visualcla/prompt_lookup.py, which csrc/lookup.hip
follows) against transformers' own PromptLookupCandidateGenerator, the acceptance rule against HF's greedy n_matches, and the refusals
that need no GPU."""
import random

import pytest
import torch

from visualcla import prompt_lookup as PL


def _hf_candidates(ids, k, ngram, eos):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos) if eos else None, num_output_tokens=k,
                                         max_matching_ngram_size=ngram, max_length=10 ** 6)
    inp = torch.tensor([ids], dtype=torch.long)
    cand, _ = gen.get_candidates(inp)
    return cand[0, len(ids):].tolist()


def _cases(n):
    rng = random.Random(1234)
    for i in range(n):
        kind = i % 4
        L = rng.randint(1, 60)
        if kind == 0:                       # small vocabulary: many matches
            ids = [rng.randint(0, 5) for _ in range(L)]
        elif kind == 1:                     # large vocabulary: mostly no match
            ids = [rng.randint(0, 10 ** 5) for _ in range(L)]
        elif kind == 2:                     # a repeated phrase with noise
            phrase = [rng.randint(0, 50) for _ in range(rng.randint(1, 8))]
            ids = []
            while len(ids) < L:
                ids += phrase if rng.random() < 0.7 else [rng.randint(0, 50)]
            ids = ids[:L]
        else:                               # eos ids sprinkled into a repeating sequence
            ids = [rng.choice([1, 2, 3, 7, 9]) for _ in range(L)]
        eos = rng.choice([[], [2], [3, 9], [rng.randint(0, 5)]])
        yield ids, rng.randint(1, 15), rng.randint(1, 3), eos


def test_draft_selection_matches_transformers():
    n = n_drafts = n_empty = n_eos_cut = 0
    for ids, k, ngram, eos in _cases(600):
        ours = PL.lookup_drafts(ids, k, ngram, eos)
        theirs = _hf_candidates(ids, k, ngram, eos)
        assert ours == theirs, (ids, k, ngram, eos, ours, theirs)
        n += 1
        n_drafts += bool(ours)
        n_empty += not ours
        n_eos_cut += bool(eos) and 0 < len(ours) < k
    assert n == 600 and n_drafts > 100 and n_empty > 100 and n_eos_cut > 10


def test_acceptance_matches_hf_n_matches():
    rng = random.Random(7)
    for _ in range(500):
        k = rng.randint(1, 15)
        row = [rng.randint(0, 3) for _ in range(k + 1)]
        am = [rng.randint(0, 3) for _ in range(k + 1)]
        # hf generation/utils.py _assisted_decoding, greedy: n_matches = ((~(candidate == selected[:, :-1])).cumsum(-1) < 1).sum()
        cand = torch.tensor([row[1:]])
        sel = torch.tensor([am])
        n_hf = int(((~(cand == sel[:, :-1])).cumsum(dim=-1) < 1).sum())
        assert PL.accepted(row, am) == n_hf


def test_lookup_step_emits_greedy_tokens():
    """the host step: emitted ids are argmax[0 .. n], cut at eos and the budget; a done state changes nothing"""
    hist, out = [5, 6, 7, 5, 6], []
    st = dict(done=0, pos=0, iterations=0, accepted=0)
    row = PL.next_row(hist, 3, 2, [2])
    assert row == [6, 7, 5, 6]
    nxt = PL.lookup_step(row, [7, 5, 9, 1], hist, out, st, budget=10, eos_ids=[2], k=3)
    assert out == [7, 5, 9] and st["pos"] == 3 and st["accepted"] == 2 and nxt[0] == 9
    nxt2 = PL.lookup_step(nxt, [2, 4, 4, 4], hist, out, st, budget=10, eos_ids=[2], k=3)
    assert out == [7, 5, 9, 2] and st["done"] == 1
    assert PL.lookup_step(nxt2, [8, 8, 8, 8], hist, out, st, budget=10, eos_ids=[2], k=3) == nxt2 and out == [7, 5, 9, 2] and st["pos"] == 4
    hist, out = [1, 2, 3], []
    st = dict(done=0, pos=0, iterations=0, accepted=0)
    PL.lookup_step([3, 4, 5], [4, 5, 6], hist, out, st, budget=2, eos_ids=[], k=2)
    assert out == [4, 5] and st["done"] == 1


def test_prompt_lookup_is_no_longer_refused_by_name():
    from transformers import GenerationConfig
    from visualcla.logits_processors import refuse_unsupported
    refuse_unsupported(GenerationConfig(prompt_lookup_num_tokens=3))


@pytest.mark.parametrize("kw, word", [
    (dict(prompt_lookup_num_tokens=16), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=0), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=3, do_sample=True), "do_sample"),
    (dict(prompt_lookup_num_tokens=3, num_beams=2), "num_beams"),
    (dict(prompt_lookup_num_tokens=3, repetition_penalty=1.2), "repetition_penalty"),
    (dict(prompt_lookup_num_tokens=3, no_repeat_ngram_size=2), "no_repeat_ngram_size"),
    (dict(prompt_lookup_num_tokens=3, min_new_tokens=4), "min_new_tokens"),
    (dict(prompt_lookup_num_tokens=3, max_time=5.0), "max_time"),
])
def test_refusal_matrix(kw, word):
    from transformers import GenerationConfig
    from visualcla.modeling_visualcla import VisualCLAModel
    with pytest.raises(ValueError, match=word):
        VisualCLAModel._refuse_lookup_conflicts(GenerationConfig(**kw), None, None, None, None)


def test_refusal_of_callbacks():
    from transformers import GenerationConfig, StoppingCriteriaList
    from visualcla.modeling_visualcla import VisualCLAModel
    gc = GenerationConfig(prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="stopping_criteria"):
        VisualCLAModel._refuse_lookup_conflicts(gc, None, StoppingCriteriaList([lambda i, s: False]), None, None)
    with pytest.raises(ValueError, match="logits_processor"):
        VisualCLAModel._refuse_lookup_conflicts(gc, [lambda i, s: s], None, None, None)
    with pytest.raises(ValueError, match="prefix_allowed_tokens_fn"):
        VisualCLAModel._refuse_lookup_conflicts(gc, None, None, lambda b, i: [0], None)
    VisualCLAModel._refuse_lookup_conflicts(gc, None, None, None, None)

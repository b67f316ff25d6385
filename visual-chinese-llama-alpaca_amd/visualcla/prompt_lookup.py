"""Host restatement of the prompt-lookup bookkeeping that csrc/lookup.hip runs on the device (one launch per verify iteration).

Draft selection is transformers' `PromptLookupCandidateGenerator.get_candidates` (generation/candidate_generator.py) without a logits
processor; acceptance is the greedy branch of `_assisted_decoding` (generation/utils.py): `n_matches` = the number of leading drafts equal to
the argmax of the row before them.  The tests hold the kernel to these functions and these functions to transformers.
"""
from __future__ import annotations

from typing import List, Sequence


def lookup_drafts(history: Sequence[int], k: int, ngram_max: int = 2, eos_ids: Sequence[int] = ()) -> List[int]:
    """Up to k draft ids for the sequence `history`: the longest tail n-gram (ngram_max .. 1) that occurs earlier with a non-empty
    continuation, its EARLIEST such occurrence, the continuation cut before the first eos id.  A match whose cut leaves nothing proposes
    nothing (transformers does not try another match then)."""
    h = [int(x) for x in history]
    L = len(h)
    eos = set(int(e) for e in eos_ids)
    for n in range(min(ngram_max, L - 1), 0, -1):
        tail = h[L - n:]
        for idx in range(0, L - n):
            if h[idx:idx + n] == tail:
                out = []
                for t in h[idx + n:min(idx + n + k, L)]:
                    if t in eos:
                        break
                    out.append(t)
                return out
    return []


def accepted(row: Sequence[int], argmax: Sequence[int]) -> int:
    """n_matches: row = [last token, d_1 .. d_k], argmax[i] = greedy choice after row[0 .. i]; drafts d_1 .. d_n are accepted"""
    n = 0
    while n < len(row) - 1 and int(row[n + 1]) == int(argmax[n]):
        n += 1
    return n


def lookup_step(row: List[int], argmax: Sequence[int], history: List[int], out: List[int], state: dict, budget: int,
                eos_ids: Sequence[int], k: int, ngram_max: int = 2, filler: int = -1) -> List[int]:
    """One iteration of vcla_lookup_step, on host lists: emits into `out` / `history`, updates state (count, done, pos, iterations,
    accepted) and returns the next row (unchanged once done)."""
    eos = set(int(e) for e in eos_ids)
    if not state["done"]:
        n = accepted(row, argmax)
        e = 0
        for i in range(n + 1):
            if len(out) >= budget:
                state["done"] = 1
                break
            t = int(argmax[i])
            out.append(t)
            history.append(t)
            e += 1
            if t in eos:
                state["done"] = 1
                break
        if len(out) >= budget:
            state["done"] = 1
        state["pos"] += e
        state["iterations"] += 1
        state["accepted"] += max(e - 1, 0)
    if state["done"]:
        return list(row)
    return next_row(history, k, ngram_max, eos_ids, filler)


def next_row(history: Sequence[int], k: int, ngram_max: int = 2, eos_ids: Sequence[int] = (), filler: int = -1) -> List[int]:
    """[last token, drafts ..., filler ...] of length k + 1 (filler < 0: the last token)"""
    last = int(history[-1])
    d = lookup_drafts(history, k, ngram_max, eos_ids)
    fill = last if filler < 0 else int(filler)
    return [last] + d + [fill] * (k - len(d))

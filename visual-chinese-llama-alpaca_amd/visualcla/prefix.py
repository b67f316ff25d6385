"""Prefix sharing for generate_many(share_prefix=True), host side: the plan.

Under causal attention the K/V rows [0, P) of a prompt depend on nothing behind P, so requests of one queue that begin with the same ids
(and, behind the first image placeholder, carry the same image) can have those rows computed once and copied.  `plan` decides, before
the first admission and from host lists alone, which request keeps a copy of its leading rows in the call's prefix pool (an ENTRY), which
entry every request reads, and how many rows that saves; `passes` orders the requests admitted at one boundary so that nobody reads rows
that are still being computed.  Nothing here knows the device (tests/test_prefix_host.py).

Terms: request indices are arrival order = admission order.  An entry is named by the request that creates it.
  match(i, c)   the common prefix, on ids, of prompts i and c; positions at or behind the first image placeholder of prompt c count only
                when both requests carry the same image (image keys compared with ==: the caller gives equal keys to equal images).
  usable(i, e)  min(match(i, creator(e)), rows(e), T_i - 1) -- one row of every prompt must run to produce logits -- or 0 when that is
                below `min_shared_rows` (a copy launch is not worth a few rows; the default 16 is a judgement, not a measurement).
  source(i)     the entry with creator < i of largest usable(i, e), the oldest on ties; None when all are 0.  P_i = usable(i, source(i)).
  creation      request c creates an entry exactly when some LATER request j would reuse at least min_shared_rows more rows from c's
                prompt than from every entry planned before c (min(match(j, c), T_j - 1) - max_e usable(j, e)), and the pool has room.
                The entry keeps rows [0, n), n = the longest such match.  c may itself read an older entry.
  lifetime      an entry lives from its creator to its last reader, in arrival order, and `slots - 1` arrivals longer: the requests of
                one boundary (at most `slots`) are prefilled in passes, not in arrival order, so a later arrival of the last reader's
                boundary may be prefilled before it.  Readers keep an entry alive however far away they are; nothing is evicted.
  room          when c is planned, the rows of the entries alive at c (their last readers as planned so far, c's would-be readers
                already moved to c) plus n must not exceed `pool_rows`.  Later creators only take readers away, so lives only shrink
                and the bound holds for the final plan.  Without room c creates nothing and its would-be readers compute their own rows
                (or read what an older entry offers): no request is refused or reordered.

Block granularity (plan(..., block_rows=16), generate_many(kv_pool_tokens=, share_blocks=True)): on the paged K/V pool a
shared prefix is not copied -- reader and creator NAME the same pool blocks -- so only whole blocks can be shared.  The plan is the plan
above with every P_i and every entry length rounded DOWN to a multiple of block_rows (a length below one block counts as 0: the request
then reads nothing and the entry, if nobody reads it, is dropped); source, creators, passes and lifetimes are otherwise unchanged, and
P_i <= T_i - 1 still holds.  The rows between the last full block and what the exact plan reuses are recomputed.  vision_needed stays the
exact plan's: a request whose image slot reaches behind its rounded P_i but whose exact plan needed no vision run takes the image
features its source's creator used (image_from[i]: that creator; equal images by value), so those rows are computed from equal inputs.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

MIN_SHARED_ROWS = 16
DEFAULT_POOL_ENTRIES = 16


@dataclass
class Entry:
    creator: int
    rows: int                   # the pool keeps rows [0, rows) of the creator's prompt
    last_reader: int            # the last request that reads it
    readers: List[int] = field(default_factory=list)


@dataclass
class PrefixPlan:
    T: List[int]
    P: List[int]                            # rows request i copies instead of computing
    source: List[Optional[int]]             # the creator of the entry it copies them from
    vision_needed: List[bool]               # the request has an image and its slot is not wholly inside [0, P_i)
    entries: Dict[int, Entry]               # creator -> entry (only entries somebody reads)
    slots: int
    pool_rows: int
    min_shared_rows: int
    denied: List[int]                       # would-be creators that found the pool full
    block_rows: int = 0                     # > 0: the plan at block granularity (P and entry lengths are multiples of it)
    image_from: List[Optional[int]] = field(default_factory=list)     # block plan: the creator whose image features request i takes, or None

    @property
    def rows_reused(self) -> int:
        return sum(self.P)

    @property
    def rows_computed(self) -> int:
        return sum(t - p for t, p in zip(self.T, self.P))

    @property
    def vision_runs(self) -> int:
        return sum(self.vision_needed)

    def live_rows_at(self, i: int) -> int:
        """pool rows held when request i is admitted (the lifetime rule of the module header)"""
        return sum(e.rows for e in self.entries.values() if e.creator <= i <= e.last_reader + self.slots - 1)

    @property
    def peak_pool_rows(self) -> int:
        return max((self.live_rows_at(e.creator) for e in self.entries.values()), default=0)


def _match(ids: np.ndarray, lens: np.ndarray, c: int, J: np.ndarray, keys: Sequence, first_img: Sequence[Optional[int]]) -> np.ndarray:
    """match(j, c) for the requests J: ids [n, Tmax] padded with -1"""
    Tc = int(lens[c])
    eq = ids[J, :Tc] == ids[c, :Tc][None, :]
    m = np.minimum(np.cumprod(eq, axis=1).sum(axis=1), lens[J])
    f = first_img[c]
    if f is not None:
        other = np.fromiter((keys[j] != keys[c] for j in J), dtype=bool, count=len(J))
        m = np.where(other, np.minimum(m, f), m)
    return m


def plan(prompts: Sequence[Sequence[int]], image_keys: Sequence, img_token_id: Optional[int], slots: int, pool_rows: Optional[int] = None,
         min_shared_rows: int = MIN_SHARED_ROWS, block_rows: Optional[int] = None) -> PrefixPlan:
    """prompts[i]: the ids of request i (one per decoder position); image_keys[i]: None, or a value equal for equal images; slots: the
    decode batch (at most that many requests share a boundary); pool_rows: the pool bound in rows (None: DEFAULT_POOL_ENTRIES entries of
    the longest prefix the queue would keep with an unbounded pool).  block_rows (None: today's plan): the plan at block granularity
    (module header)."""
    if block_rows is not None:
        if isinstance(block_rows, bool) or not isinstance(block_rows, int) or block_rows < 1:
            raise ValueError(f"prefix.plan: block_rows must be a positive integer (got {block_rows!r})")
        return _to_blocks(plan(prompts, image_keys, img_token_id, slots, pool_rows, min_shared_rows), prompts, img_token_id, int(block_rows))
    if pool_rows is None:
        free = _plan(prompts, image_keys, img_token_id, slots, 1 << 40, min_shared_rows)
        free.pool_rows = DEFAULT_POOL_ENTRIES * max((e.rows for e in free.entries.values()), default=0)
        # a plan that never met the bound is the plan under every bound it fits
        return free if free.peak_pool_rows <= free.pool_rows else _plan(prompts, image_keys, img_token_id, slots, free.pool_rows, min_shared_rows)
    return _plan(prompts, image_keys, img_token_id, slots, int(pool_rows), min_shared_rows)


def _plan(prompts, image_keys, img_token_id, slots, pool_rows, min_shared_rows) -> PrefixPlan:
    n = len(prompts)
    msr = max(int(min_shared_rows), 1)
    lens = np.array([len(p) for p in prompts], dtype=np.int64)
    Tmax = int(lens.max()) if n else 0
    ids = np.full((n, max(Tmax, 1)), -1, dtype=np.int64)
    for i, p in enumerate(prompts):
        ids[i, :len(p)] = np.asarray(p, dtype=np.int64)
    first_img: List[Optional[int]] = [None] * n
    last_img: List[Optional[int]] = [None] * n
    if img_token_id is not None:
        is_img = ids == img_token_id
        for i in np.nonzero(is_img.any(axis=1))[0]:
            pos = np.nonzero(is_img[i])[0]
            first_img[i], last_img[i] = int(pos[0]), int(pos[-1])
    # a match of min_shared_rows rows needs equal leading ids: only the requests of one such family are ever compared
    family: Dict[bytes, List[int]] = {}
    for i in range(n):
        if lens[i] > msr:                                        # (T_i - 1 >= min_shared_rows, or nothing of it can be shared)
            family.setdefault(ids[i, :msr].tobytes(), []).append(i)
    later_of: Dict[int, np.ndarray] = {}
    for members in family.values():
        arr = np.asarray(members, dtype=np.int64)
        for k, i in enumerate(members[:-1]):
            later_of[i] = arr[k + 1:]
    cap = lens - 1                                               # one row of every prompt must run
    best = np.zeros(n, dtype=np.int64)                           # usable rows from the best entry so far
    src = np.full(n, -1, dtype=np.int64)
    rows_of: Dict[int, int] = {}
    denied: List[int] = []
    for c in range(n):
        J = later_of.get(c)
        if J is None:
            continue
        m = np.minimum(_match(ids, lens, c, J, image_keys, first_img), cap[J])
        would = m - best[J] >= msr
        if not would.any():
            continue
        keep = int(m[would].max())
        use = np.minimum(m, keep)
        use = np.where(use >= msr, use, 0)
        moved = use > best[J]                                    # strictly longer: ties stay with the older entry
        src_if = src.copy()
        src_if[J[moved]] = c
        held = np.nonzero(src_if >= 0)[0]
        last = dict(zip(src_if[held].tolist(), held.tolist()))   # ascending: the last reader of every entry that has one
        live = sum(r for e, r in rows_of.items() if e in last and last[e] + slots - 1 >= c)
        if live + keep > pool_rows:
            denied.append(c)
            continue
        rows_of[c] = keep
        best[J[moved]] = use[moved]
        src = src_if
    entries: Dict[int, Entry] = {}
    for j in range(n):
        if src[j] >= 0:
            e = entries.setdefault(int(src[j]), Entry(int(src[j]), rows_of[int(src[j])], j))
            e.last_reader = j
            e.readers.append(j)
    P = [int(best[j]) if src[j] >= 0 else 0 for j in range(n)]
    source = [int(src[j]) if src[j] >= 0 else None for j in range(n)]
    vision = [image_keys[j] is not None and not (last_img[j] is not None and last_img[j] < P[j]) for j in range(n)]
    return PrefixPlan([int(t) for t in lens], P, source, vision, entries, int(slots), int(pool_rows), int(min_shared_rows), denied)


def _to_blocks(pl: PrefixPlan, prompts, img_token_id: Optional[int], br: int) -> PrefixPlan:
    """the exact plan `pl` at block granularity: P_i and entry lengths rounded down to multiples of br; who reads whom does not change"""
    n = len(pl.T)
    P = [p // br * br for p in pl.P]
    source = [s if p > 0 else None for s, p in zip(pl.source, P)]
    entries: Dict[int, Entry] = {}
    for j in range(n):
        if source[j] is not None:
            c = source[j]
            e = entries.setdefault(c, Entry(c, pl.entries[c].rows // br * br, j))
            e.last_reader = j
            e.readers.append(j)
    image_from: List[Optional[int]] = [None] * n
    vision = list(pl.vision_needed)
    if img_token_id is not None:
        for j in range(n):
            if pl.source[j] is not None and pl.P[j] > 0 and not pl.vision_needed[j]:
                last = max((k for k, t in enumerate(prompts[j]) if t == img_token_id), default=None)
                if last is not None and last >= P[j]:             # the slot reaches behind the shared blocks: its rows need the image features
                    image_from[j], vision[j] = (source[j], False) if source[j] is not None else (None, True)
    return PrefixPlan(list(pl.T), P, source, vision, entries, pl.slots, pl.pool_rows, pl.min_shared_rows, list(pl.denied), br, image_from)


def passes(pl: PrefixPlan, admitted: Sequence[int]) -> List[List[int]]:
    """The requests admitted at one boundary, in the passes that prefill them: a request whose source entry exists already (its creator was
    admitted at an earlier boundary) or that has none goes into pass 1; one whose source entry is created by a request of this boundary
    goes into the pass behind its creator's.  Arrival order inside a pass."""
    here = set(admitted)
    depth: Dict[int, int] = {}
    for i in sorted(admitted):                                   # a creator always arrives before its readers
        s = pl.source[i]
        depth[i] = depth[s] + 1 if (s is not None and s in here) else 1
    out: List[List[int]] = [[] for _ in range(max(depth.values(), default=0))]
    for i in sorted(admitted):
        out[depth[i] - 1].append(i)
    return out

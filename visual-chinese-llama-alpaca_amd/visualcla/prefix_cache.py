"""A prefix cache that outlives the call, host side: the index behind generate_many(share_prefix=True, prefix_cache=...) (DESIGN.md
section 7g).

The plan of visualcla/prefix.py shares rows between the requests of ONE queue and forgets them when the call returns.  This index
addresses K/V rows BY CONTENT, so that a later call -- the next queue of questions about the same images, under the same system prompt
-- finds them again.  Nothing here knows the device (tests/test_prefix_cache_host.py): the index deals in block numbers; the pool tensor,
the pixel tensors of the images and the tables of the copies belong to `PrefixCache` at the end of this file, which imports torch
only inside its methods.

Terms
  block        BLOCK_ROWS = 16 consecutive prompt rows [16 k, 16 k + 16) of some prompt (16 is prefix.MIN_SHARED_ROWS: what is not worth a
               copy launch inside a queue is not worth a block either, and 16 rows start 16-byte aligned for every head dim).
  chain key    (parent block, the block's 16 ids, image): `parent` is the pool index of the block that holds the 16 rows before it (-1 for
               k = 0); `image` is None until the chain has reached the first image placeholder of the prompt (the block contains it or
               lies behind it), from there on the cache's id for the prompt's image.  Under causal attention the rows [0, 16 k) of a
               prompt are a function of exactly the chain of its first k keys, so equal chains hold equal rows.  A parent is named by
               its pool index: that is unambiguous because a block is never evicted before its resident children.
  lookup       once per request at the start of a call: walk the chain while its keys are resident, at most floor((T - 1) / 16) blocks
               (one row of every prompt must run to produce logits).  The blocks found are PINNED until end_call and stamped with the
               call's number.
  insertion    after an admission pass, per member in arrival order: walk the chain over the FULL blocks of the prompt,
               [0, 16 floor(T / 16)); a resident block is stamped, a missing one is allocated (so a block two members both miss is
               inserted once, by the earlier arrival).  Every block an insertion batch walks or allocates is held until the batch is
               handed to the device (`hold`): the copies of one batch go out in one launch, so no block of it may be evicted -- and
               handed out a second time -- inside the batch, and a parent must outlive the moment its child is registered.
  allocation   a free block first; else the evictable block of oldest stamp, ties to the deeper block, then to the lower index.
               Evictable: not pinned, not held, no resident children.  With nothing evictable the rest of that chain is skipped and
               counted (`insert_skipped`, in blocks): no request is refused or delayed.
  images       the index counts, per image id, the blocks that name it; an id nobody names any more is reported by `dead_images()` so
               that the owner of the pixel tensors drops them with the last block.
"""
from __future__ import annotations

from typing import Dict, Hashable, List, Optional, Sequence, Set, Tuple

BLOCK_ROWS = 16
STAT_KEYS = ("calls", "cache_rows_reused", "cache_blocks_inserted", "cache_evictions", "cache_insert_skipped", "invalidated")


def first_image_pos(ids: Sequence[int], img_token_id: Optional[int]) -> Optional[int]:
    if img_token_id is None:
        return None
    for p, t in enumerate(ids):
        if t == img_token_id:
            return p
    return None


class PrefixCacheIndex:
    def __init__(self, n_blocks: int, block_rows: int = BLOCK_ROWS):
        if int(n_blocks) < 0 or int(block_rows) < 1:
            raise ValueError(f"a prefix cache needs n_blocks >= 0 and block_rows >= 1 (got {n_blocks}, {block_rows})")
        self.n_blocks = int(n_blocks)
        self.block_rows = int(block_rows)
        self.stats = {k: 0 for k in STAT_KEYS}
        self.call = 0
        self._reset()

    def _reset(self) -> None:
        n = self.n_blocks
        self.key_of: List[Optional[tuple]] = [None] * n          # block -> its chain key (None: free)
        self.block_of: Dict[tuple, int] = {}                     # chain key -> block
        self.parent: List[int] = [-1] * n
        self.depth: List[int] = [0] * n                          # k of the block in its chain
        self.children: List[int] = [0] * n                       # resident children
        self.stamp: List[int] = [0] * n
        self.free: List[int] = list(range(n - 1, -1, -1))        # popped from the end: lowest index first
        self.pinned: Set[int] = set()
        self.image_refs: Dict[Hashable, int] = {}
        self._dead: List[Hashable] = []

    # ------------------------------------------------------------------ state
    @property
    def used(self) -> int:
        return self.n_blocks - len(self.free)

    def resident(self, block: int) -> bool:
        return self.key_of[block] is not None

    def clear(self) -> None:
        """forgets every block (the counters stay)"""
        dead = list(self.image_refs)
        self._reset()
        self._dead = dead

    def invalidate(self) -> None:
        """the rows no longer describe the model (a rebuilt context): clear, and count it"""
        self.clear()
        self.stats["invalidated"] += 1

    def dead_images(self) -> List[Hashable]:
        """image ids whose last block left since the previous call of this method"""
        dead, self._dead = [i for i in self._dead if i not in self.image_refs], []
        return dead

    # ------------------------------------------------------------------ a call
    def begin_call(self) -> int:
        self.call += 1
        self.stats["calls"] += 1
        self.pinned.clear()
        return self.call

    def end_call(self) -> None:
        self.pinned.clear()

    def _keys(self, ids: Sequence[int], image: Hashable, first_img: Optional[int], n: int):
        """the chain keys of blocks 0 .. n - 1 of a prompt, minus the parent (which only the walk knows)"""
        R = self.block_rows
        for k in range(n):
            reached = image is not None and first_img is not None and first_img < (k + 1) * R
            yield tuple(int(t) for t in ids[k * R:(k + 1) * R]), (image if reached else None)

    def lookup(self, ids: Sequence[int], image: Hashable = None, first_img: Optional[int] = None, pin: bool = True) -> List[int]:
        """-> the resident chain of the prompt, as pool blocks in chain order, at most floor((T - 1) / 16) of them: C = 16 * len(result).
        pin: the blocks are pinned until end_call and stamped with the call's number (False: a query that changes nothing)."""
        out: List[int] = []
        parent = -1
        for blk_ids, img in self._keys(ids, image, first_img, (len(ids) - 1) // self.block_rows if len(ids) else 0):
            b = self.block_of.get((parent, blk_ids, img))
            if b is None:
                break
            out.append(b)
            parent = b
        if pin:
            for b in out:
                self.pinned.add(b)
                self.stamp[b] = self.call
        return out

    def count_reused(self, rows: int) -> None:
        """rows a request actually took from the cache (`combine` decides; a lookup alone reuses nothing)"""
        self.stats["cache_rows_reused"] += int(rows)

    def _evict_one(self, hold: Set[int]) -> Optional[int]:
        best = None
        for b in range(self.n_blocks):
            if self.key_of[b] is None or self.children[b] or b in self.pinned or b in hold:
                continue
            rank = (self.stamp[b], -self.depth[b], b)
            if best is None or rank < best[0]:
                best = (rank, b)
        if best is None:
            return None
        b = best[1]
        key = self.key_of[b]
        del self.block_of[key]
        self.key_of[b] = None
        if self.parent[b] >= 0:
            self.children[self.parent[b]] -= 1
        img = key[2]
        if img is not None:
            self.image_refs[img] -= 1
            if not self.image_refs[img]:
                del self.image_refs[img]
                self._dead.append(img)
        self.stats["cache_evictions"] += 1
        return b

    def insert(self, ids: Sequence[int], image: Hashable = None, first_img: Optional[int] = None, hold: Optional[Set[int]] = None) -> List[Tuple[int, int]]:
        """Walks the chain of the prompt's full blocks; -> [(k, block)] for the blocks allocated now, in chain order: the caller copies rows
        [16 k, 16 k + 16) of the prompt into `block`.  hold: the blocks of the current insertion batch (updated in place)."""
        hold = hold if hold is not None else set()
        out: List[Tuple[int, int]] = []
        parent = -1
        n = len(ids) // self.block_rows
        for k, (blk_ids, img) in enumerate(self._keys(ids, image, first_img, n)):
            key = (parent, blk_ids, img)
            b = self.block_of.get(key)
            if b is None:
                b = self.free.pop() if self.free else self._evict_one(hold)
                if b is None:
                    self.stats["cache_insert_skipped"] += n - k
                    break
                self.key_of[b], self.block_of[key] = key, b
                self.parent[b], self.depth[b], self.children[b] = parent, k, 0
                if parent >= 0:
                    self.children[parent] += 1
                if img is not None:
                    self.image_refs[img] = self.image_refs.get(img, 0) + 1
                self.stats["cache_blocks_inserted"] += 1
                out.append((k, b))
            self.stamp[b] = self.call
            hold.add(b)
            parent = b
        return out


def combine(plan, cached_rows: Sequence[int], prompts: Sequence[Sequence[int]], has_image: Sequence[bool], img_token_id: Optional[int]):
    """The plan of a queue (prefix.PrefixPlan, made exactly as without a cache) and the rows C_i the cache offers every request ->
    (P, from_cache, vision_needed): request i reuses P_i = max(C_i, Pplan_i) rows from ONE source -- the cache when C_i >= Pplan_i (and
    C_i > 0), else its plan entry -- and needs the vision stack when it has an image whose placeholders are not wholly inside [0, P_i)."""
    P, from_cache, vision = [], [], []
    for i, c in enumerate(cached_rows):
        c = int(c)
        use = c > 0 and c >= plan.P[i]
        p = c if use else plan.P[i]
        last_img = None
        if has_image[i] and img_token_id is not None:
            for pos in range(len(prompts[i]) - 1, -1, -1):
                if prompts[i][pos] == img_token_id:
                    last_img = pos
                    break
        P.append(p)
        from_cache.append(use)
        vision.append(bool(has_image[i]) and not (last_img is not None and last_img < p))
    return P, from_cache, vision


def _fingerprints(flat) -> List[tuple]:
    """one fingerprint per row of `flat` [n, N] (images in the model dtype), to be found again in a LATER call: two wrapping int64 sums over
    the elements' bit patterns, plain and weighted by position.  Integer addition is associative, so the value does not depend on how the
    reduction is split -- a floating-point sum over the stacked images (what _image_keys uses inside one call) changes with the number of
    images stacked beside it, and an image of an earlier queue would be missed.  x + 0 first: -0.0 == 0.0 by value, so both print alike."""
    import torch
    bits = (flat + 0).view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[flat.element_size()]).to(torch.int64)
    w = torch.arange(1, flat.shape[1] + 1, device=flat.device, dtype=torch.int64)
    return [tuple(fp) for fp in torch.stack([bits.sum(1), (bits * w).sum(1)], dim=1).tolist()]


class PrefixCache:
    """The device side of the index: the pool [n_blocks, L, 2, H, 16, d] in the model dtype, the pixel tensors of the images its blocks
    name, and the bookkeeping of one generate_many call.  Made by model.new_prefix_cache(max_tokens); `nbytes`, `block_rows`, `stats`
    (accumulated over calls), `used_blocks`, `clear()`.  Not thread-safe: one call at a time, as the model itself."""

    def __init__(self, model, max_tokens: int):
        if isinstance(max_tokens, bool) or int(max_tokens) < BLOCK_ROWS:
            raise ValueError(f"max_tokens must be at least one block of {BLOCK_ROWS} rows (got {max_tokens!r})")
        self.model = model
        self.index = PrefixCacheIndex(int(max_tokens) // BLOCK_ROWS)
        self.pool = None
        self._epoch = None
        self._images: Dict[int, tuple] = {}                      # image id -> (shape, fingerprint, pixel values in the model dtype)
        self._by_print: Dict[tuple, List[int]] = {}              # (shape, fingerprint) -> image ids
        self._next_image = 0
        self.peak_used_blocks = 0
        self._ensure(count=False)

    block_rows = BLOCK_ROWS

    @property
    def n_blocks(self) -> int:
        return self.index.n_blocks

    @property
    def max_tokens(self) -> int:
        return self.index.n_blocks * BLOCK_ROWS

    @property
    def used_blocks(self) -> int:
        return self.index.used

    @property
    def stats(self) -> dict:
        return dict(self.index.stats, used_blocks=self.index.used, images=len(self._images))

    @property
    def nbytes(self) -> int:
        return 0 if self.pool is None else self.pool.numel() * self.pool.element_size()

    def clear(self) -> None:
        """forget every block and every image (the pool and the counters stay)"""
        self.index.clear()
        self.index.dead_images()
        self._images.clear()
        self._by_print.clear()

    def _ensure(self, count: bool = True) -> None:
        """the pool, in the model's current dtype on its device; a context rebuilt since the rows were written (a dtype switch,
        enable_fp8_decode, set_image_size, a device move) empties the cache"""
        import torch
        m = self.model
        if self._epoch == m._session_epoch and self.pool is not None and self.pool.dtype == m._dtype and self.pool.device == m._device:
            return
        if count and self._epoch is not None:
            self.index.invalidate()
            self.clear()
        t = m.config.text_config
        H = t["num_attention_heads"]
        shape = (self.index.n_blocks, t["num_hidden_layers"], 2, H, BLOCK_ROWS, t["hidden_size"] // H)
        if self.pool is None or self.pool.dtype != m._dtype or self.pool.device != m._device:
            self.pool = None                                     # (release before the new allocation)
            self.pool = torch.empty(shape, dtype=m._dtype, device=m._device)
        self._epoch = m._session_epoch

    # ------------------------------------------------------------------ images, by value
    def _image_ids(self, reqs, keys) -> List[Optional[int]]:
        """keys[i]: the queue's own image key of request i (_image_keys: equal for equal images) -> the cache's id of every request's image.
        As _prefix_plan compares: one fingerprint per distinct image buckets them, an exact comparison after the cast to the model dtype
        decides (one copy back each).  Unknown images get a new id and are kept -- until the end of the call when no block names them."""
        import torch
        m = self.model
        reps = sorted({k for k in keys if k is not None})        # the representative request of every distinct image
        id_of: Dict[int, int] = {}
        by_shape: Dict[tuple, List[int]] = {}
        for r in reps:
            by_shape.setdefault(tuple(reqs[r]["px"].shape), []).append(r)
        for shape, members in by_shape.items():
            flat = torch.stack([reqs[r]["px"].to(m._dtype) for r in members]).flatten(1)
            prints = _fingerprints(flat)
            pairs = [(k, c) for k, fp in enumerate(prints) for c in self._by_print.get((shape, tuple(fp)), ())]
            if pairs:
                a = flat[torch.tensor([k for k, _ in pairs], device=flat.device)]
                b = torch.stack([self._images[c][2] for _, c in pairs])
                for (k, c), same in zip(pairs, (a == b).all(dim=1).tolist()):
                    if same:
                        id_of.setdefault(members[k], c)
            for k, r in enumerate(members):
                if r not in id_of:
                    self._next_image += 1
                    id_of[r] = self._next_image
                    self._images[id_of[r]] = (shape, tuple(prints[k]), flat[k])
                    self._by_print.setdefault((shape, tuple(prints[k])), []).append(id_of[r])
                    self._new_images.append(id_of[r])
        return [None if k is None else id_of[k] for k in keys]

    def _drop_image(self, i: int) -> None:
        shape, fp, _ = self._images.pop(i)
        ids = self._by_print[(shape, fp)]
        ids.remove(i)
        if not ids:
            del self._by_print[(shape, fp)]

    # ------------------------------------------------------------------ one generate_many call
    def begin(self, reqs, plan, keys, prompts, img_token_id):
        """Lookup for every request, once, before the first admission -> the call's state: P / from_cache / vision_needed (`combine`), the
        chain of blocks each request reads, its image id and first placeholder (what the insertions key on)."""
        self._ensure()
        idx = self.index
        idx.begin_call()
        self._new_images: List[int] = []
        self._before = dict(idx.stats)
        image = self._image_ids(reqs, keys)
        first = [first_image_pos(p, img_token_id) if image[i] is not None else None for i, p in enumerate(prompts)]
        chains = [idx.lookup(p, image[i], first[i]) for i, p in enumerate(prompts)]
        P, from_cache, vision = combine(plan, [len(c) * BLOCK_ROWS for c in chains], prompts, [k is not None for k in keys], img_token_id)
        idx.count_reused(sum(p for p, c in zip(P, from_cache) if c))
        return dict(cache=self, prompts=prompts, image=image, first=first, chains=chains, P=P, from_cache=from_cache, vision=vision)

    def read_entries(self, state, members, slot_of):
        """the table that copies the cached rows of the requests `members` into their slots: [(block, slot, row0)]"""
        return [(b, slot_of[i], k * BLOCK_ROWS) for i in members if state["from_cache"][i]
                for k, b in enumerate(state["chains"][i][:state["P"][i] // BLOCK_ROWS])]

    def insert_entries(self, state, members, slot_of):
        """after an admission pass: the full prompt blocks of its members that are not resident, in arrival and chain order, as the table
        that copies them out of the slots"""
        hold: Set[int] = set()
        out = []
        for i in members:
            for k, b in self.index.insert(state["prompts"][i], state["image"][i], state["first"][i], hold):
                out.append((b, slot_of[i], k * BLOCK_ROWS))
        self.peak_used_blocks = max(self.peak_used_blocks, self.index.used)
        return out

    def end(self) -> dict:
        """unpins, drops the images nobody names, and -> the four counters of this call"""
        import torch
        idx = self.index
        idx.end_call()
        for i in idx.dead_images():
            if i in self._images:
                self._drop_image(i)
        for i in self._new_images:
            if i in self._images:
                if i not in idx.image_refs:
                    self._drop_image(i)
                else:                                            # a row of the call's stacked copy: keep the image alone
                    shape, fp, px = self._images[i]
                    self._images[i] = (shape, fp, px.clone())
        self._new_images = []
        keys = ("cache_rows_reused", "cache_blocks_inserted", "cache_evictions", "cache_insert_skipped")
        return {k: idx.stats[k] - self._before[k] for k in keys}

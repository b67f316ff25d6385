"""The prefix cache that outlives the call, host side (visualcla/prefix_cache.py): chain keys and lookup against a
brute-force value on Python lists, the bounded cache's invariants on random traffic, the eviction order on hand-made sequences, the
counters, and the combination with the plan of a queue.  No GPU."""
import random

import pytest

from visualcla import prefix as P
from visualcla import prefix_cache as PC

IMG, IMG_S, IMG_E = 900, 901, 902          # <img_token>, <img>, </img>
R = PC.BLOCK_ROWS


def _slot(q=8):
    return [IMG_S] + [IMG] * q + [IMG_E]


def _first(p):
    return p.index(IMG) if IMG in p else None


def _match(p, kp, c, kc):
    """match of visualcla/prefix.py, written out: the common prefix on ids; positions at or behind the first placeholder of c count only
    under the same image"""
    m = 0
    while m < min(len(p), len(c)) and p[m] == c[m]:
        m += 1
    if IMG in c and kp != kc:
        m = min(m, c.index(IMG))
    return m


def _brute(p, kp, inserted):
    return max((R * (min(_match(p, kp, c, kc), len(p) - 1) // R) for c, kc in inserted), default=0)


def _random_queue(rng, n):
    """prompts over a small vocabulary with planted common heads and two images; -> [(ids, image id or None)]"""
    heads = [[1] + [rng.randrange(3, 7) for _ in range(rng.choice((15, 20, 33, 47)))] for _ in range(3)]
    out = []
    for _ in range(n):
        ids = list(rng.choice(heads))
        key = None
        if rng.random() < 0.6:
            key = rng.choice(("A", "B"))
            ids = ids[:rng.choice((len(ids), 9, 16))] + _slot(rng.choice((8, 13)))
        ids += [rng.randrange(3, 7) for _ in range(rng.randrange(0, 40))]
        if rng.random() < 0.2 and out:                           # a strict extension, or a copy, of an earlier prompt
            base, key = rng.choice(out)
            ids = list(base) + [rng.randrange(3, 7) for _ in range(rng.choice((0, 1, 16, 21)))]
        out.append((ids, key))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_lookup_equals_brute_force_with_unbounded_capacity(seed):
    rng = random.Random(seed)
    queue = _random_queue(rng, 40)
    idx = PC.PrefixCacheIndex(4096)
    idx.begin_call()
    inserted = []
    hit = 0
    for ids, key in queue:
        got = idx.lookup(ids, key, _first(ids), pin=False)
        want = _brute(ids, key, inserted)
        assert R * len(got) == want, (ids, key, got, want)
        assert got == idx.lookup(ids, key, _first(ids), pin=True)
        hit += want > 0
        new = idx.insert(ids, key, _first(ids))
        inserted.append((ids, key))
        # every full block of the prompt is resident now, the new ones behind the resident ones, and a second insertion adds nothing
        assert [k for k, _ in new] == list(range(len(ids) // R - len(new), len(ids) // R))
        assert idx.insert(ids, key, _first(ids)) == []
        assert R * len(idx.lookup(ids, key, _first(ids), pin=False)) == R * ((len(ids) - 1) // R)
    assert hit >= 10 and idx.stats["cache_evictions"] == 0 and idx.stats["cache_insert_skipped"] == 0
    assert idx.used == idx.stats["cache_blocks_inserted"] == len(idx.block_of)
    # the other image under equal ids: the chain ends in front of the block that holds the first placeholder
    ids = [1] + [5] * 20 + _slot() + [4] * 30
    idx.insert(ids, "A", _first(ids))
    assert R * len(idx.lookup(ids, "B", _first(ids), pin=False)) == R * (_first(ids) // R) == 16
    assert R * len(idx.lookup(ids, "A", _first(ids), pin=False)) == R * ((len(ids) - 1) // R)


def _check_structure(idx, capacity):
    assert idx.used <= capacity and idx.used == len(idx.block_of) == sum(k is not None for k in idx.key_of)
    kids = [0] * capacity
    for b, key in enumerate(idx.key_of):
        if key is None:
            continue
        assert idx.block_of[key] == b
        par = key[0]
        assert par == idx.parent[b]
        if par >= 0:                                             # no block outlives its parent: a parent is evicted behind its children
            assert idx.key_of[par] is not None and idx.depth[b] == idx.depth[par] + 1, (b, par)
            kids[par] += 1
        else:
            assert idx.depth[b] == 0
    assert kids == [idx.children[b] if idx.key_of[b] is not None else 0 for b in range(capacity)]
    refs = {}
    for key in idx.block_of:
        if key[2] is not None:
            refs[key[2]] = refs.get(key[2], 0) + 1
    assert refs == idx.image_refs


@pytest.mark.parametrize("capacity,seed", [(4, 0), (7, 1), (16, 2), (16, 3), (40, 4)])
def test_bounded_cache_invariants_on_random_traffic(capacity, seed):
    rng = random.Random(100 + seed)
    idx = PC.PrefixCacheIndex(capacity)
    pool = _random_queue(rng, 30)
    evictions = 0
    for call in range(12):
        idx.begin_call()
        queue = [rng.choice(pool) for _ in range(rng.randrange(1, 9))]
        pinned = {}
        for ids, key in queue:
            chain = idx.lookup(ids, key, _first(ids))
            assert len(chain) <= (len(ids) - 1) // R
            for k, b in enumerate(chain):                        # every chain lookup returns is resident, and it is this prompt's chain
                got = idx.key_of[b]
                assert got is not None and got[1] == tuple(ids[k * R:(k + 1) * R]) and got[0] == (chain[k - 1] if k else -1)
                assert idx.stamp[b] == idx.call
                pinned[b] = got
        for at in range(0, len(queue), 3):                       # admission passes of up to three members
            hold = set()
            before = idx.stats["cache_evictions"]
            dst = []
            for ids, key in queue[at:at + 3]:
                new = idx.insert(ids, key, _first(ids), hold)
                dst += [b for _, b in new]
                for k, b in new:
                    assert idx.key_of[b][1] == tuple(ids[k * R:(k + 1) * R])
            assert len(dst) == len(set(dst)), "one block handed out twice inside one copy launch"
            evictions += idx.stats["cache_evictions"] - before
            _check_structure(idx, capacity)
            for b, key in pinned.items():                        # a pinned block is never evicted
                assert idx.key_of[b] == key
        idx.end_call()
        assert not idx.pinned
    assert idx.stats["cache_blocks_inserted"] - idx.stats["cache_evictions"] == idx.used
    assert evictions == idx.stats["cache_evictions"] and (capacity > 16 or evictions > 0)


def _ids(tag, n):
    return [tag * 1000 + k for k in range(n)]


def test_eviction_order_by_stamp_then_depth_then_index():
    idx = PC.PrefixCacheIndex(4)
    A, B, C = _ids(1, 48), _ids(2, 16), _ids(3, 32)
    idx.begin_call()
    assert idx.insert(A) == [(0, 0), (1, 1), (2, 2)]             # free blocks first, lowest index first
    idx.end_call()
    idx.begin_call()
    assert idx.insert(B) == [(0, 3)]
    idx.end_call()
    idx.begin_call()
    # the oldest stamp among the blocks without resident children: A's leaf, then the block that became a leaf by that
    assert idx.insert(C) == [(0, 2), (1, 1)]
    assert idx.stats["cache_evictions"] == 2 and len(idx.lookup(A + [0], pin=False)) == 1 and len(idx.lookup(B + [0], pin=False)) == 1
    idx.end_call()
    # ties: equal stamps go to the deeper block, then to the lower index
    idx = PC.PrefixCacheIndex(4)
    X, Y, Z = _ids(4, 32), _ids(5, 32), _ids(6, 48)
    idx.begin_call()
    assert idx.insert(X) == [(0, 0), (1, 1)] and idx.insert(Y) == [(0, 2), (1, 3)]
    idx.end_call()
    idx.begin_call()
    assert idx.insert(Z) == [(0, 1), (1, 3), (2, 0)]             # x1 and y1 tie on depth: the lower index; then y1 is deeper than x0; then x0 before y0
    idx.end_call()
    # a pinned chain is passed over, whatever its stamp; so is everything the insertion batch holds
    idx = PC.PrefixCacheIndex(4)
    idx.begin_call()
    idx.insert(X)
    idx.end_call()
    idx.begin_call()
    idx.insert(Y)
    idx.end_call()
    idx.begin_call()
    assert idx.lookup(X + [0]) == [0, 1]                         # pinned, and stamped with this call
    assert idx.insert(Z) == [(0, 3), (1, 2)]                     # y1, y0; then only X (pinned) and Z's own blocks (held) are left
    assert idx.stats["cache_insert_skipped"] == 1 and idx.stats["cache_evictions"] == 2
    idx.end_call()
    idx.begin_call()
    assert idx.insert(_ids(7, 16)) == [(0, 1)]                   # unpinned: X and Z carry equal stamps, x1 and z1 equal depth, x1 the lower index
    idx.end_call()


def test_insert_skip_invalidation_and_image_counters():
    idx = PC.PrefixCacheIndex(2)
    idx.begin_call()
    p = [1] + [5] * 7 + _slot() + [4] * 60                       # 78 ids: four full blocks, the placeholders in the first two
    assert idx.insert(p, 7, _first(p)) == [(0, 0), (1, 1)]       # one batch: nothing of it is evictable for its own tail
    assert idx.stats["cache_insert_skipped"] == 2 and idx.stats["cache_evictions"] == 0 and idx.used == 2
    assert idx.image_refs == {7: 2}
    idx.end_call()
    idx.begin_call()
    assert idx.lookup(p, 7, _first(p), pin=False) == [0, 1] and idx.lookup(p, 8, _first(p), pin=False) == []
    q = _ids(9, 32)
    assert idx.insert(q) == [(0, 1), (1, 0)]                     # the leaf first, then its parent
    assert idx.dead_images() == [7] and idx.image_refs == {} and idx.dead_images() == []
    assert idx.stats["cache_evictions"] == 2 and idx.stats["invalidated"] == 0
    idx.invalidate()
    assert idx.stats["invalidated"] == 1 and idx.used == 0 and idx.lookup(q + [0], pin=False) == [] and idx.stats["cache_blocks_inserted"] == 4
    assert idx.insert(q) == [(0, 0), (1, 1)]
    # a cache without blocks: everything is skipped, nothing fails
    none = PC.PrefixCacheIndex(0)
    none.begin_call()
    assert none.insert(q) == [] and none.lookup(q, pin=True) == [] and none.stats["cache_insert_skipped"] == 2


def test_combination_with_the_plan_on_the_queue_of_the_device_tests():
    from oracle import visualcla_oracle as O
    from tests.test_gpu_prefix import IMAGE_OF, _queue
    cfg = O.cfg_tiny()
    prompts = [r[0][0].tolist() for r in _queue(cfg)]
    tok = cfg.img_token_id
    T = [len(p) for p in prompts]
    has = [k is not None for k in IMAGE_OF]
    plan = P.plan(prompts, IMAGE_OF, tok, 4)
    idx = PC.PrefixCacheIndex(1024)
    first = [p.index(tok) if (tok in p and has[i]) else None for i, p in enumerate(prompts)]
    # call 1, a cold cache: the plan alone
    idx.begin_call()
    C = [R * len(idx.lookup(p, IMAGE_OF[i], first[i])) for i, p in enumerate(prompts)]
    assert C == [0] * 14
    assert PC.combine(plan, C, prompts, has, tok) == (plan.P, [False] * 14, plan.vision_needed)
    for i, p in enumerate(prompts):
        idx.insert(p, IMAGE_OF[i], first[i])
    idx.end_call()
    # call 2: every prompt finds its own full blocks in front of its last row
    idx.begin_call()
    C = [R * len(idx.lookup(p, IMAGE_OF[i], first[i])) for i, p in enumerate(prompts)]
    assert C == [R * ((t - 1) // R) for t in T]
    Pc, from_cache, vision = PC.combine(plan, C, prompts, has, tok)
    assert Pc == [max(c, q) for c, q in zip(C, plan.P)]
    assert from_cache == [c > 0 and c >= q for c, q in zip(C, plan.P)] and any(from_cache) and all(p < t for p, t in zip(Pc, T))
    last = [max(k for k, t in enumerate(p) if t == tok) if tok in p else None for p in prompts]
    assert vision == [has[i] and not (last[i] is not None and last[i] < Pc[i]) for i in range(14)]
    assert sum(vision) <= sum(plan.vision_needed) and sum(Pc) > sum(plan.P)
    # request 12 carries the ids of request 1 under another image: in a cache that saw only request 1 its chain ends at the placeholder's block
    solo = PC.PrefixCacheIndex(64)
    solo.begin_call()
    solo.insert(prompts[1], IMAGE_OF[1], first[1])
    assert R * len(solo.lookup(prompts[12], IMAGE_OF[12], first[12])) == R * (first[12] // R)
    assert R * len(solo.lookup(prompts[1], IMAGE_OF[1], first[1])) == R * ((T[1] - 1) // R)


def test_prefix_cache_object_on_a_stand_in_model_images_by_value():
    """PrefixCache needs a model only for its shape, dtype, device and epoch: on the CPU with a stand-in, the images by value (a clone is the
    same image, another image under equal ids is not), their release with the last block, and the epoch rule"""
    import torch
    from types import SimpleNamespace
    m = SimpleNamespace(_session_epoch=1, _dtype=torch.float32, _device=torch.device("cpu"),
                        config=SimpleNamespace(text_config=dict(num_attention_heads=2, num_hidden_layers=2, hidden_size=8)))
    cache = PC.PrefixCache(m, max_tokens=64)
    assert cache.n_blocks == 4 and tuple(cache.pool.shape) == (4, 2, 2, 2, 16, 4) and cache.nbytes == 64 * 2 * 2 * 8 * 4 and cache.block_rows == 16
    g = torch.Generator().manual_seed(0)
    img_a, img_b = torch.randn(3, 4, 4, generator=g), torch.randn(3, 4, 4, generator=g)
    p = [1] + [5] * 7 + _slot() + [4] * 20                       # 38 ids: two full blocks, both name the image
    q = [1] + [6] * 39                                           # text only
    reqs = [dict(px=img_a), dict(px=img_b), dict(px=None)]
    prompts = [p, p, q]
    plan = P.plan(prompts, [0, 1, None], IMG, 4)

    def call(reqs, keys):
        st = cache.begin(reqs, plan, keys, prompts, IMG)
        slot_of = {0: 0, 1: 1, 2: 2}
        reads = cache.read_entries(st, [0, 1, 2], slot_of)
        writes = cache.insert_entries(st, [0, 1, 2], slot_of)
        return st, reads, writes, cache.end()
    st, reads, writes, stats = call(reqs, [0, 1, None])
    assert st["P"] == plan.P and reads == [] and stats["cache_rows_reused"] == 0
    # four blocks for six: request 0's two, request 1's two (another image from row 9 on), nothing left for the text request
    assert writes == [(0, 0, 0), (1, 0, 16), (2, 1, 0), (3, 1, 16)] and stats["cache_insert_skipped"] == 2 and cache.stats["images"] == 2
    # clones of the pixel tensors are the same images; the image that was b is now request 0's
    reqs2 = [dict(px=img_b.clone()), dict(px=img_a.clone()), dict(px=None)]
    st, reads, writes, stats = call(reqs2, [0, 1, None])
    assert st["chains"] == [[2, 3], [0, 1], []] and st["P"] == [32, 32, 0] and st["from_cache"] == [True, True, False] and st["vision"] == [False, False, False]
    assert reads == [(2, 0, 0), (3, 0, 16), (0, 1, 0), (1, 1, 16)] and writes == [] and stats["cache_rows_reused"] == 64 and cache.stats["images"] == 2
    # a third image under the same ids finds nothing, and (everything else unpinned) pushes the oldest chain out, leaf first
    img_c = img_a + 1
    st, reads, writes, stats = call([dict(px=img_c), dict(px=None), dict(px=None)], [0, None, None])
    assert st["chains"][0] == [] and stats["cache_evictions"] == 4 and cache.stats["images"] == 1 and cache.used_blocks == 4
    assert len(cache._images) == 1 and torch.equal(next(iter(cache._images.values()))[2], img_c.flatten())
    # a rebuilt context: the next call starts from an empty cache, once
    m._session_epoch = 2
    st, reads, writes, stats = call([dict(px=img_c), dict(px=None), dict(px=None)], [0, None, None])
    assert cache.stats["invalidated"] == 1 and st["chains"] == [[], [], []] and stats["cache_rows_reused"] == 0 and cache.stats["calls"] == 4
    cache.clear()
    assert cache.used_blocks == 0 and cache.stats["images"] == 0 and cache.stats["invalidated"] == 1


def test_an_image_is_found_again_whatever_is_stacked_beside_it():
    """the fingerprint of an image must not depend on the queue it arrives in: a later queue carries other images beside it, and fewer or
    more of them (a floating-point sum over the stacked images is split by the stack's shape).  Integer sums over the bit patterns are exact."""
    import torch
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(1)
    imgs = [torch.randn(3, 56, 56, generator=g) * 3 for _ in range(9)]
    for dt in (torch.float32, torch.bfloat16):
        flat = torch.stack(imgs).to(dt).flatten(1)
        full = PC._fingerprints(flat)
        assert len(set(full)) == 9 and all(isinstance(x, int) for fp in full for x in fp)
        for pick in ([0], [4], [8, 0], [2, 3, 4], [8, 7, 6, 5, 4, 3, 2]):
            assert PC._fingerprints(flat[pick]) == [full[k] for k in pick], (dt, pick)
        z = flat[:1].clone()
        z[0, :5] = 0.0
        nz = z.clone()
        nz[0, :5] = -0.0
        assert torch.equal(z, nz) and PC._fingerprints(z) == PC._fingerprints(nz) != full[:1]
    # through the cache: the first queue brings four images, the second one of them alone, the third two others among new ones
    m = SimpleNamespace(_session_epoch=1, _dtype=torch.float32, _device=torch.device("cpu"),
                        config=SimpleNamespace(text_config=dict(num_attention_heads=2, num_hidden_layers=2, hidden_size=8)))
    cache = PC.PrefixCache(m, max_tokens=1024)
    p = [1] + [5] * 7 + _slot() + [4] * 20

    def call(pictures):
        n = len(pictures)
        st = cache.begin([dict(px=x.clone()) for x in pictures], P.plan([p] * n, list(range(n)), IMG, 4), list(range(n)), [p] * n, IMG)
        cache.insert_entries(st, list(range(n)), {i: i for i in range(n)})
        cache.end()
        return st["image"], [len(c) for c in st["chains"]]
    first, found = call(imgs[:4])
    assert len(set(first)) == 4 and found == [0] * 4
    assert call([imgs[2]]) == ([first[2]], [2])
    image, found = call([imgs[5], imgs[3], imgs[6], imgs[0], imgs[7], imgs[8], imgs[1]])
    assert [image[1], image[3], image[6]] == [first[3], first[0], first[1]] and found == [0, 2, 0, 2, 0, 0, 2]
    assert len(set(image) | set(first)) == 8 and cache.stats["images"] == 8

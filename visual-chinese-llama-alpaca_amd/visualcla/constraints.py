"""Per-request token constraints of generate_many as data (csrc/constrain.hip): the request keys `allowed_token_ids`,
`banned_token_ids` and `choices` become small token automata, and the closed queue becomes ONE flat table, built before the first
admission and uploaded once.

  allowed_token_ids  one ALLOW node whose edges loop back to itself
  banned_token_ids   one DENY node: its edges are the banned ids, the state never moves
  choices            a trie of allow nodes.  A node that completes a choice also has one edge per eos id of the request's config into an
                     END node, beside its edges into longer choices; END allows only the eos ids and loops to itself

Automata that are equal by value (for choices: the eos tuple included) share their nodes.  Edges are sorted by token inside a node.
Records: node = (edge0, n_edges, deny, 0), edge = (token, next), int32 each -- vcla_cs_node / vcla_cs_edge.  Needs no device."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

KEYS = ("allowed_token_ids", "banned_token_ids", "choices")
MAX_NODES = 65536           # VCLA_CS_MAX_NODES
MAX_EDGES = 1 << 20         # VCLA_CS_MAX_EDGES
MAX_VOCAB = 1 << 19         # VCLA_CS_MAX_VOCAB: the bitmask of a row in 64 KiB of LDS

Spec = Tuple[str, tuple]    # (key, ids) / ("choices", choices): sorted, without duplicates


def _ids(i: int, key: str, x, what: str) -> List[int]:
    if hasattr(x, "tolist"):
        if getattr(x, "dtype", None) is not None and (getattr(x.dtype, "is_floating_point", False) or "float" in str(x.dtype) or "bool" in str(x.dtype)):
            raise ValueError(f"request {i}: {key} must hold integer token ids (got {x.dtype})")
        x = x.tolist()
    if not isinstance(x, (list, tuple)):
        raise ValueError(f"request {i}: {key} must be {what} (got {type(x).__name__})")
    for t in x:
        if isinstance(t, bool) or not isinstance(t, int):
            raise ValueError(f"request {i}: {key} must hold integer token ids (got {t!r})")
    return list(x)


def parse(i: int, r: dict) -> Optional[Spec]:
    """the constraint of request dict `r` -> its spec, None without one.  Refuses, by request index: more than one of the three keys, any of
    them beside target_ids, an empty list or choice, anything but integers."""
    given = [k for k in KEYS if r.get(k) is not None]
    if not given:
        return None
    if len(given) > 1:
        raise ValueError(f"request {i}: {' and '.join(given)} exclude each other (at most one constraint per request)")
    key = given[0]
    if r.get("target_ids") is not None:
        raise ValueError(f"request {i}: {key} beside target_ids (a forced request takes its targets whatever a constraint allows)")
    if key != "choices":
        ids = _ids(i, key, r[key], "a list of token ids")
        if not ids:
            raise ValueError(f"request {i}: {key} is empty")
        return key, tuple(sorted(set(ids)))
    ch = r[key].tolist() if hasattr(r[key], "tolist") else r[key]
    if not isinstance(ch, (list, tuple)) or not ch:
        raise ValueError(f"request {i}: choices is empty" if isinstance(ch, (list, tuple)) else f"request {i}: choices must be a list of lists of token ids")
    out = []
    for c in ch:
        if not hasattr(c, "tolist") and not isinstance(c, (list, tuple)):
            raise ValueError(f"request {i}: choices must be a list of lists of token ids (got an entry {c!r})")
        ids = _ids(i, "choices", c, "a list of lists of token ids")
        if not ids:
            raise ValueError(f"request {i}: choices holds an empty choice")
        out.append(tuple(ids))
    return key, tuple(sorted(set(out)))


def check(i: int, spec: Optional[Spec], vocab_size: int, eos: Sequence[int], floor: int, no_repeat_ngram_size: int) -> None:
    """what depends on the request's resolved config: eos its eos ids, floor its min-token floor (min_new_tokens / min_length)"""
    if spec is None:
        return
    key, val = spec
    flat = val if key != "choices" else [t for c in val for t in c]
    if not all(0 <= t < vocab_size for t in flat):
        raise ValueError(f"request {i}: {key} outside the vocabulary 0..{vocab_size - 1}")
    if vocab_size > MAX_VOCAB:
        raise ValueError(f"request {i}: {key} with vocab_size={vocab_size} (the token set of a row is a bitmask in LDS: at most {MAX_VOCAB})")
    if key == "choices":
        if not eos:
            raise ValueError(f"request {i}: choices needs an eos_token_id in the request's config (a completed choice ends with it)")
        if no_repeat_ngram_size and int(no_repeat_ngram_size) > 0:
            raise ValueError(f"request {i}: choices beside no_repeat_ngram_size={no_repeat_ngram_size} (a ban could empty the set a choice leaves)")
        if floor > 0:
            raise ValueError(f"request {i}: choices beside a min-token floor (min_new_tokens / min_length = {floor}): the floor would ban the only allowed token")
    if key == "allowed_token_ids" and floor > 0 and set(val) <= set(eos):
        raise ValueError(f"request {i}: allowed_token_ids are all eos ids while a min-token floor of {floor} is on (min_new_tokens / min_length): nothing is left to take")


class Table:
    """nodes [[edge0, n_edges, deny, 0]], edges [[token, next]], roots[i]: request i's root node (-1: unconstrained), automata: distinct ones"""
    __slots__ = ("nodes", "edges", "roots", "automata", "constrained")

    def __init__(self):
        self.nodes: List[List[int]] = []
        self.edges: List[List[int]] = []
        self.roots: List[int] = []
        self.automata = 0
        self.constrained = 0

    # ---- a host walk (the tests' model of the two kernels)
    def node_set(self, s: int):
        """-> (tokens of the node's edges, deny)"""
        e0, n, deny, _ = self.nodes[s]
        return {t for t, _ in self.edges[e0:e0 + n]}, bool(deny)

    def keeps(self, s: int, tok: int) -> bool:
        toks, deny = self.node_set(s)
        return (tok in toks) != deny

    def step(self, s: int, tok: int) -> int:
        e0, n, deny, _ = self.nodes[s]
        if deny:
            return s
        for t, nx in self.edges[e0:e0 + n]:
            if t == tok:
                return nx
        return s

    def tensors(self, device):
        import torch
        return (torch.tensor(self.nodes, dtype=torch.int32).view(-1, 4).to(device), torch.tensor(self.edges, dtype=torch.int32).view(-1, 2).to(device))

    def stats(self) -> dict:
        return dict(constrained_requests=self.constrained, automaton_nodes=len(self.nodes), automaton_edges=len(self.edges))


def _add(tb: Table, spec: Spec, eos: tuple) -> int:
    key, val = spec
    base = len(tb.nodes)
    if key != "choices":
        tb.nodes.append([len(tb.edges), len(val), int(key == "banned_token_ids"), 0])
        tb.edges.extend([t, base] for t in val)
        return base
    trie: List[Dict[int, int]] = [{}]                             # local node -> {token: local child}
    terminal = [False]
    for c in val:
        s = 0
        for t in c:
            if t not in trie[s]:
                trie[s][t] = len(trie)
                trie.append({})
                terminal.append(False)
            s = trie[s][t]
        terminal[s] = True
    end = len(trie)                                               # END: only the eos ids, looping
    for s, kids in enumerate(trie):
        out = {t: base + k for t, k in kids.items()}
        if terminal[s]:
            for e in eos:
                out.setdefault(e, base + end)                     # (an eos id that also continues a longer choice: the request ends on it either way)
        tb.nodes.append([len(tb.edges), len(out), 0, 0])
        tb.edges.extend([t, out[t]] for t in sorted(out))
    tb.nodes.append([len(tb.edges), len(eos), 0, 0])
    tb.edges.extend([e, base + end] for e in eos)
    return base


def build(specs: Sequence[Optional[Spec]], eos_of: Sequence[Sequence[int]]) -> Optional[Table]:
    """the table of a queue: specs[i] / eos_of[i] are request i's spec (None: unconstrained) and eos ids.  None when no request has a spec.
    Refuses a table beyond MAX_NODES / MAX_EDGES by name."""
    if all(s is None for s in specs):
        return None
    tb, seen = Table(), {}
    for i, spec in enumerate(specs):
        if spec is None:
            tb.roots.append(-1)
            continue
        eos = tuple(sorted(set(int(e) for e in eos_of[i]))) if spec[0] == "choices" else ()
        k = (spec, eos)
        if k not in seen:
            seen[k] = _add(tb, spec, eos)
            if len(tb.nodes) > MAX_NODES or len(tb.edges) > MAX_EDGES:
                raise ValueError(f"generate_many: the constraints of requests 0..{i} need {len(tb.nodes)} automaton nodes and {len(tb.edges)} edges "
                                 f"(caps: VCLA_CS_MAX_NODES = {MAX_NODES}, VCLA_CS_MAX_EDGES = {MAX_EDGES})")
        tb.roots.append(seen[k])
        tb.constrained += 1
    tb.automata = len(seen)
    return tb


def from_items(constraints, n_items: int) -> List[Optional[dict]]:
    """chat_many's `constraints`: one entry per item, None or {one of the three keys: ids}"""
    if len(constraints) != n_items:
        raise ValueError(f"chat_many: constraints has {len(constraints)} entries for {n_items} items")
    out = []
    for i, c in enumerate(constraints):
        if c is not None and (not isinstance(c, dict) or len(c) != 1 or next(iter(c)) not in KEYS):
            raise ValueError(f"chat_many: constraints[{i}] must be None or a dict with exactly one of {list(KEYS)}")
        out.append(c)
    return out

"""Per-request token constraints of generate_many, host side: the refusals by request index before any device call,
the ABI of the new entries, and the automaton builder of visualcla/constraints.py against a brute-force walk.  No GPU."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest
import torch


class _Constraints:
    """visualcla.constraints, imported at first use: without the module every test fails on its own, at what it checks"""
    def __getattr__(self, name):
        from visualcla import constraints
        return getattr(constraints, name)


K = _Constraints()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vcla_constrain_rows", "vcla_constrain_advance", "vcla_llama_decode_slots_constrained")
V = 100


def _bare_model():
    """a VisualCLAModel without weights or device: what the argument checks touch"""
    from visualcla.modeling_visualcla import VisualCLAModel
    m = VisualCLAModel.__new__(VisualCLAModel)
    m._device = torch.device("cpu")
    m.generation_config = None
    m._ctx = None
    return m


# ------------------------------------------------------------------ 1. refusals
def test_request_keys_are_refused_by_index_before_any_device_call():
    m = _bare_model()
    ids = torch.arange(3, 9)
    req = lambda **kw: dict(input_ids=ids, **kw)                 # noqa: E731
    with pytest.raises(ValueError, match=r"request 3: allowed_token_ids and choices exclude each other"):
        m._inflight_request(3, req(allowed_token_ids=[4], choices=[[4]]))
    with pytest.raises(ValueError, match=r"request 1: allowed_token_ids and banned_token_ids exclude"):
        m._inflight_request(1, req(allowed_token_ids=[4], banned_token_ids=[5]))
    for key, val in (("allowed_token_ids", [4]), ("banned_token_ids", [4]), ("choices", [[4]])):
        with pytest.raises(ValueError, match=rf"request 2: {key} beside target_ids"):
            m._inflight_request(2, req(target_ids=[4, 5], **{key: val}), 0)
    with pytest.raises(ValueError, match=r"request 4: allowed_token_ids is empty"):
        m._inflight_request(4, req(allowed_token_ids=[]))
    with pytest.raises(ValueError, match=r"request 4: banned_token_ids is empty"):
        m._inflight_request(4, req(banned_token_ids=[]))
    with pytest.raises(ValueError, match=r"request 5: choices is empty"):
        m._inflight_request(5, req(choices=[]))
    with pytest.raises(ValueError, match=r"request 5: choices holds an empty choice"):
        m._inflight_request(5, req(choices=[[4], []]))
    for bad in ([1.5], [True], ["a"], torch.tensor([1.5])):
        with pytest.raises(ValueError, match=r"request 6: allowed_token_ids must hold integer"):
            m._inflight_request(6, req(allowed_token_ids=bad))
    with pytest.raises(ValueError, match=r"request 6: choices must"):
        m._inflight_request(6, req(choices=[[4, 2.0]]))
    with pytest.raises(ValueError, match=r"request 6: choices must"):
        m._inflight_request(6, req(choices=[4, 5]))
    # what is accepted: lists, tuples, tensors; duplicates collapse
    assert m._inflight_request(0, req(allowed_token_ids=torch.tensor([9, 4, 9])))["constraint"] == ("allowed_token_ids", (4, 9))
    assert m._inflight_request(0, req(banned_token_ids=(7,)))["constraint"] == ("banned_token_ids", (7,))
    assert m._inflight_request(0, req(choices=[[5, 6], [5], [5, 6]]))["constraint"] == ("choices", ((5,), (5, 6)))
    assert m._inflight_request(0, req())["constraint"] is None
    # every existing refusal stays: an unknown key is still unknown
    with pytest.raises(ValueError, match=r"request 0: unknown keys \['allowed_ids'\]"):
        m._inflight_request(0, req(allowed_ids=[1]))


def test_config_dependent_refusals_by_index():
    from transformers import GenerationConfig
    from visualcla.modeling_visualcla import VisualCLAModel as M
    m = _bare_model()
    ids = torch.arange(3, 9)

    def table(gc, **key):
        return M._constraint_table([m._inflight_request(0, dict(input_ids=ids)), m._inflight_request(1, dict(input_ids=ids, **key))], [gc, gc], V)
    greedy = GenerationConfig(do_sample=False, eos_token_id=2)
    for key, val in (("allowed_token_ids", [4, V]), ("banned_token_ids", [-1]), ("choices", [[4], [5, V]])):
        with pytest.raises(ValueError, match=rf"request 1: {key} outside the vocabulary 0\.\.{V - 1}"):
            table(greedy, **{key: val})
    with pytest.raises(ValueError, match=r"request 1: choices needs an eos_token_id"):
        table(GenerationConfig(do_sample=False, eos_token_id=None), choices=[[4]])
    with pytest.raises(ValueError, match=r"request 1: choices beside no_repeat_ngram_size=3"):
        table(GenerationConfig(do_sample=False, eos_token_id=2, no_repeat_ngram_size=3), choices=[[4]])
    with pytest.raises(ValueError, match=r"request 1: choices beside a min-token floor"):
        table(GenerationConfig(do_sample=False, eos_token_id=2, min_new_tokens=2), choices=[[4]])
    with pytest.raises(ValueError, match=r"request 1: allowed_token_ids are all eos ids while a min-token floor"):
        table(GenerationConfig(do_sample=False, eos_token_id=[2, 3], min_new_tokens=2), allowed_token_ids=[3, 2])
    # allowed beside a floor is fine when something but the eos is left; the lists alone need no eos
    tb = table(GenerationConfig(do_sample=False, eos_token_id=[2, 3], min_new_tokens=2), allowed_token_ids=[3, 2, 7])
    assert tb.roots == [-1, 0] and tb.stats() == dict(constrained_requests=1, automaton_nodes=1, automaton_edges=3)
    assert table(GenerationConfig(do_sample=False, eos_token_id=None), banned_token_ids=[5]).nodes == [[0, 1, 1, 0]]
    assert M._constraint_table([m._inflight_request(0, dict(input_ids=ids))], [greedy], V) is None


def test_chat_many_constraints_argument():
    from visualcla import modeling_utils
    with pytest.raises(ValueError, match="constraints has 1 entries for 0 items"):
        modeling_utils.chat_many(None, [], constraints=[None])
    with pytest.raises(ValueError, match=r"constraints\[1\] must be None or a dict with exactly one of"):
        K.from_items([None, dict(allowed_token_ids=[1], choices=[[1]])], 2)
    with pytest.raises(ValueError, match=r"constraints\[0\] must be"):
        K.from_items([dict(words=["A"])], 1)
    assert K.from_items([None, dict(choices=[[1]])], 2) == [None, dict(choices=[[1]])]


# ------------------------------------------------------------------ 2. the ABI
def test_new_symbols_are_declared_exported_and_bound():
    from visualcla import _lib as L
    header = open(os.path.join(ROOT, "include", "visualcla_hip.h")).read()
    assert re.search(r"#define\s+VCLA_ABI_VERSION\s+5\b", header)
    for name, val in (("VCLA_CS_MAX_NODES", L.CS_MAX_NODES), ("VCLA_CS_MAX_EDGES", L.CS_MAX_EDGES), ("VCLA_CS_MAX_VOCAB", L.CS_MAX_VOCAB)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)\b", header).group(1)) == val, name
    assert (K.MAX_NODES, K.MAX_EDGES, K.MAX_VOCAB) == (L.CS_MAX_NODES, L.CS_MAX_EDGES, L.CS_MAX_VOCAB)
    assert (L.CS_MAX_VOCAB + 31) // 32 * 4 == 64 * 1024          # the bitmask of the largest vocabulary is 64 KiB of LDS
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1], name
    # the new entry is the logprobs one plus one pointer
    assert len(L.SYMBOLS["vcla_llama_decode_slots_constrained"][1]) == len(L.SYMBOLS["vcla_llama_decode_slots_logprobs"][1]) + 1


def test_struct_sizes_and_offsets_match_c(tmp_path):
    from visualcla import _lib as L
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    structs = (("vcla_cs_node", L.CsNode), ("vcla_cs_edge", L.CsEdge), ("vcla_constrain_args", L.ConstrainArgs))
    exprs, want = [], []
    for cname, S in structs:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(S))
        for f, _ in S._fields_:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(S, f).offset)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "visualcla_hip.h"\nint main(void) { size_t v[] = {' + ", ".join(exprs) +
                   '}; for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and got[0] == 16 and C.sizeof(L.CsEdge) == 8


def test_constrain_args_helper_checks_its_buffers():
    from visualcla import _lib as L
    nodes, edges, state = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="nodes must be"):
        L.constrain_args(nodes.long(), edges, state)
    with pytest.raises(ValueError, match="edges must be"):
        L.constrain_args(nodes, edges.view(2, 3), state)
    with pytest.raises(ValueError, match="state must be"):
        L.constrain_args(nodes, edges, state.float())
    with pytest.raises(ValueError, match="VCLA_CS_MAX_NODES"):
        L.constrain_args(torch.zeros(L.CS_MAX_NODES + 1, 4, dtype=torch.int32), edges, state)
    a = L.constrain_args(nodes, edges, state)
    assert (a.nodes, a.edges, a.state, a.n_nodes, a.n_edges) == (nodes.data_ptr(), edges.data_ptr(), state.data_ptr(), 1, 3)


# ------------------------------------------------------------------ 3. the builder against brute force
def _brute(choices, eos, hist):
    """the set allowed behind `hist` (no eos in it yet): next tokens of the consistent choices, plus the eos ids at a complete choice"""
    n = len(hist)
    out = {c[n] for c in choices if len(c) > n and list(c[:n]) == hist}
    if any(list(c) == hist for c in choices):
        out |= set(eos)
    return out


def _walk_all(tb, root, choices, eos):
    """every history that spells a prefix of a choice: the node's set is the brute-force set; behind an eos the END node allows only eos ids"""
    seen = 0
    for c in choices:
        s, hist = root, []
        for t in list(c) + [None]:
            toks, deny = tb.node_set(s)
            assert not deny and toks == _brute(choices, eos, hist), (choices, eos, hist)
            e0, n, _, pad = tb.nodes[s]
            assert [x for x, _ in tb.edges[e0:e0 + n]] == sorted(toks) and pad == 0          # sorted by token, no token twice
            seen += 1
            if t is None:
                break
            assert tb.keeps(s, t) and not tb.keeps(s, max(max(map(max, choices)), max(eos)) + 1)
            s = tb.step(s, t)
            hist.append(t)
        for e in eos:                                            # the request ends on the eos; the state is an END node all the same
            if e not in {c2[len(c)] for c2 in choices if len(c2) > len(c) and list(c2[:len(c)]) == list(c)}:
                end = tb.step(s, e)
                assert tb.node_set(end) == (set(eos), False) and all(tb.step(end, x) == end for x in eos)
        assert tb.step(s, 10 ** 6) == s                          # a token that is no edge does not move the state
    return seen


def test_builder_on_planted_choice_sets():
    eos = (2, 90)
    choices = [[5, 6, 7], [5, 6], [5, 8], [9], [5, 6], [11, 12, 13, 14]]      # shared prefixes, a prefix of another, one token, a duplicate
    tb = K.build([K.parse(0, dict(choices=choices))], [list(eos)])
    assert tb.roots == [0] and tb.constrained == 1 and tb.automata == 1
    # trie nodes: root, 5, 56, 567, 58, 9, 11, 11-12, 11-12-13, 11-12-13-14, END
    assert len(tb.nodes) == 11 and tb.stats()["automaton_edges"] == len(tb.edges)
    assert _walk_all(tb, 0, [tuple(c) for c in choices], eos) > 0
    s56 = tb.step(tb.step(0, 5), 6)                              # terminal AND internal
    assert tb.node_set(s56) == ({7, 2, 90}, False)
    assert tb.node_set(tb.step(0, 9)) == ({2, 90}, False)


@pytest.mark.parametrize("seed", range(8))
def test_builder_random_choice_sets_vs_brute_force(seed):
    rng = random.Random(seed)
    eos = tuple(sorted(rng.sample(range(0, 6), rng.choice([1, 1, 2, 3]))))
    alphabet = list(range(6, 6 + rng.choice([2, 3, 8])))          # a small alphabet: many shared prefixes
    choices = [tuple(rng.choice(alphabet) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 14))]
    choices.append(choices[0][:1])                               # a one-token choice that is a prefix of another (or its duplicate)
    choices.append(choices[-2])                                  # a duplicate
    # two other automata in front: the roots are offsets into one table
    specs = [K.parse(0, dict(allowed_token_ids=[7, 3, 7])), None, K.parse(2, dict(banned_token_ids=[1])), K.parse(3, dict(choices=[list(c) for c in choices]))]
    tb = K.build(specs, [list(eos)] * 4)
    assert tb.roots[:3] == [0, -1, 1] and tb.roots[3] == 2 and tb.constrained == 3
    assert tb.node_set(0) == ({3, 7}, False) and tb.step(0, 7) == 0 and tb.step(0, 4) == 0
    assert tb.node_set(1) == ({1}, True) and tb.step(1, 1) == 1 and tb.step(1, 5) == 1 and tb.keeps(1, 5) and not tb.keeps(1, 1)
    _walk_all(tb, tb.roots[3], sorted(set(choices)), eos)
    assert all(0 <= nx < len(tb.nodes) and e0 + n <= len(tb.edges) and n >= 1 for e0, n, _, _ in tb.nodes for _, nx in tb.edges[e0:e0 + n])
    nodes, edges = tb.tensors("cpu")
    assert nodes.dtype == edges.dtype == torch.int32 and tuple(nodes.shape) == (len(tb.nodes), 4) and tuple(edges.shape) == (len(tb.edges), 2)


def test_equal_automata_share_nodes_and_the_eos_tuple_is_part_of_equality():
    four = [[10], [11], [12, 13], [12]]
    specs = [K.parse(i, dict(choices=four if i % 2 == 0 else [list(c) for c in reversed(four)])) for i in range(16)]
    tb = K.build(specs, [[2]] * 16)
    assert len(set(tb.roots)) == 1 and tb.automata == 1 and tb.constrained == 16
    one = K.build(specs[:1], [[2]])
    assert (tb.nodes, tb.edges) == (one.nodes, one.edges)         # sixteen requests, one automaton
    other = K.build(specs[:2], [[2], [2, 3]])                    # the same choices under another eos tuple: not the same automaton
    assert other.roots[0] != other.roots[1] and other.automata == 2 and len(other.nodes) == 2 * len(one.nodes)
    assert K.build(specs[:2], [[3, 2], [2, 3, 2]]).automata == 1  # a tuple is compared as a set
    # the lists do not read the eos ids: equal lists under different eos tuples share
    lists = K.build([K.parse(0, dict(allowed_token_ids=[4, 5])), K.parse(1, dict(allowed_token_ids=[5, 4])), K.parse(2, dict(banned_token_ids=[4, 5]))], [[2], [3], [2]])
    assert lists.roots == [0, 0, 1] and lists.nodes == [[0, 2, 0, 0], [2, 2, 1, 0]]
    assert K.build([None, None], [[2], [2]]) is None


def test_caps_are_refused_by_name():
    many = K.parse(0, dict(choices=[[t] for t in range(K.MAX_NODES)]))          # MAX_NODES children + root + END
    with pytest.raises(ValueError, match=r"VCLA_CS_MAX_NODES = 65536"):
        K.build([many], [[2]])
    wide = [K.parse(i, dict(allowed_token_ids=list(range(i, i + 50000)))) for i in range(21)]      # 21 distinct lists of 50000 ids: 1.05 M edges
    with pytest.raises(ValueError, match=r"requests 0\.\.20 need .* VCLA_CS_MAX_EDGES = 1048576"):
        K.build(wide, [[2]] * 21)
    assert K.build(wide[:20], [[2]] * 20).stats()["automaton_edges"] == 10 ** 6

"""Chat sessions, the parts that need no GPU: the planning and recording rules of visualcla/session.py on host lists, the prompt-prefix
assumption the feature rests on, the refusals, the C ABI."""
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restated(sess_ids, sess_key, new_ids, span, key):
    """the rule in three lines: common prefix when the image is the session's, capped at T - 1; the vision stack is skipped when an image's slot ends inside it"""
    P = next((i for i, (a, b) in enumerate(zip(sess_ids, new_ids)) if a != b), min(len(sess_ids), len(new_ids))) if sess_key == key else 0
    P = min(P, len(new_ids) - 1)
    return P, key is not None and span is not None and span[1] <= P


def test_plan_reuse_cases():
    from visualcla.session import image_slot_span, plan_reuse
    IMG = 99
    prompt = [1, 5, 6, 90] + [IMG] * 4 + [91, 7, 8, 9]
    span = image_slot_span(prompt, IMG)
    assert span == (4, 8) and image_slot_span([1, 2, 3], IMG) is None and image_slot_span(prompt, None) is None
    sess = prompt + [20, 21, 22]                                    # the prompt, then generated ids
    assert plan_reuse([], None, prompt, span, "a") == (0, False)                       # empty session
    assert plan_reuse(sess, "a", sess + [30, 31], span, "a") == (len(sess), True)      # a later turn: everything reused, no vision stack
    assert plan_reuse(sess, "a", sess + [30, 31], span, "b") == (0, False)             # another image
    assert plan_reuse(sess, "a", sess + [30, 31], None, None) == (0, False)            # no image now, one then
    assert plan_reuse(sess, None, sess + [30], None, None) == (len(sess), False)       # text-only conversation: nothing to skip
    assert plan_reuse(sess, "a", sess, span, "a") == (len(sess) - 1, True)             # equal: the T - 1 cap, one row runs
    assert plan_reuse(sess, "a", sess[:10], span, "a") == (9, True)                    # shorter than the session's ids
    assert plan_reuse(sess, "a", sess[:13] + [77, 78], span, "a") == (13, True)        # diverges inside the generated rows
    assert plan_reuse(sess, "a", prompt[:6] + [55] + prompt[7:], span, "a") == (6, False)   # diverges inside the slot: the image embeddings are needed
    assert plan_reuse(sess, "a", prompt[:8], span, "a") == (7, False)                  # the cap cuts into the slot
    assert plan_reuse(sess, "a", [2] + sess[1:], span, "a") == (0, False)              # diverges at once
    assert plan_reuse(sess, "a", [1], None, "a") == (0, False)                         # a one-token prompt


def test_plan_reuse_random_against_the_restated_rule():
    from visualcla.session import plan_reuse
    rng = random.Random(7)
    seen = set()
    for _ in range(300):
        n = rng.randint(0, 40)
        sess = [rng.randint(1, 4) for _ in range(n)]
        T = rng.randint(1, 45)
        keep = rng.randint(0, min(n, T))
        new = sess[:keep] + [rng.randint(1, 4) for _ in range(T - keep)]
        skey = rng.choice([None, "a", "b"]) if n else None
        key = rng.choice([None, "a", "a", skey])
        span = None
        if key is not None:
            a = rng.randint(0, T - 1)
            span = (a, rng.randint(a + 1, T))
        got = plan_reuse(sess, skey, new, span, key)
        assert got == _restated(sess, skey, new, span, key), (sess, skey, new, span, key)
        assert 0 <= got[0] <= T - 1 and sess[:got[0]] == new[:got[0]]
        seen.add((got[0] > 0, got[1]))
    assert seen == {(False, False), (True, False), (True, True)}


def test_record_rule():
    from visualcla.session import plan_reuse, record_ids
    prompt = [1, 4, 5, 6]
    assert record_ids(prompt, [10, 11, 12]) == prompt + [10, 11]          # the last returned token was never fed: no row
    assert record_ids(prompt, [10]) == prompt
    # an eos in the middle of a 32-step chunk: generate() returns up to the eos; the rows the loop wrote behind it are not recorded ...
    chunk, eos = [10, 11, 2, 13, 14, 15], 2
    returned = chunk[:chunk.index(eos) + 1]
    held = record_ids(prompt, returned)
    assert held == prompt + [10, 11]
    # ... so the next turn (the response re-enters the prompt without its eos) reuses exactly the recorded rows and overwrites the rest
    nxt = prompt + [10, 11, 40, 41]
    assert plan_reuse(held, None, nxt, None, None) == (len(held), False)


class _CharTok:
    """tiny deterministic tokenizer: one id per character, special strings map to single ids (as tests/test_host_cpu.py)"""
    bos_token, img_start_token, img_end_token, img_token = "<s>", "<img>", "</img>", "<img_token>"

    def __call__(self, text, return_tensors=None, add_special_tokens=False):
        ids, i = [], 0
        spec = {"<s>": 1, "<img>": 300, "</img>": 301, "<img_token>": 303}
        while i < len(text):
            for k, v in spec.items():
                if text.startswith(k, i):
                    ids.append(v)
                    i += len(k)
                    break
            else:
                ids.append(3 + (ord(text[i]) % 250))
                i += 1
        return SimpleNamespace(input_ids=torch.tensor([ids]), attention_mask=torch.ones(1, len(ids), dtype=torch.int64))


def test_turn_one_prompt_is_a_prefix_of_turn_two():
    """the assumption the feature rests on: encoding_text only appends"""
    from visualcla.modeling_utils import encoding_text
    from visualcla.session import image_slot_span, plan_reuse, record_ids
    tok = _CharTok()
    p1 = encoding_text([], "what is this?", 4, tok).input_ids[0].tolist()
    hist = [{"type": "instruction", "value": "what is this?", "first_instruction": True}, {"type": "response", "value": "a cat"}]
    p2 = encoding_text(hist, "which colour?", 4, tok).input_ids[0].tolist()
    assert len(p2) > len(p1) and p2[:len(p1)] == p1
    # with a tokenizer that maps the response back to the generated ids the whole first turn is reused, the image slot included
    resp = tok("a cat").input_ids[0].tolist()
    held = record_ids(p1, resp + [2])                     # the eos is returned, never fed
    assert plan_reuse(held, "img", p2, image_slot_span(p2, 303), "img") == (len(p1) + len(resp), True)


def test_session_refusals_by_name():
    from visualcla.session import Session, session_conflicts
    ok = SimpleNamespace(num_beams=1, num_return_sequences=1, prompt_lookup_num_tokens=None)
    assert session_conflicts(ok, 1, False, False) == []
    assert session_conflicts(SimpleNamespace(), 1, False, False) == []
    bad = session_conflicts(SimpleNamespace(num_beams=4, num_return_sequences=2, prompt_lookup_num_tokens=3), 2, True, True)
    text = ", ".join(bad)
    for name in ("batch size 2", "num_beams=4", "num_return_sequences=2", "prompt_lookup_num_tokens=3", "image_at_head=True", "e4m3 K/V cache"):
        assert name in text, (name, text)
    assert len(bad) == 6
    model = SimpleNamespace(config=SimpleNamespace(text_config={"max_position_embeddings": 64}))
    for cap in (1, 65, 0):
        with pytest.raises(ValueError, match="max_tokens"):
            Session(model, max_tokens=cap)


def test_generate_and_chat_take_a_session():
    import inspect
    import visualcla
    from visualcla import modeling_utils
    assert "Session" in visualcla.__all__ and visualcla.Session is visualcla.session.Session
    assert "session" in inspect.signature(visualcla.VisualCLAModel.generate).parameters
    assert callable(visualcla.VisualCLAModel.new_session)
    for fn in (modeling_utils.chat, modeling_utils.chat_in_stream):
        p = inspect.signature(fn).parameters
        assert p["session"].default is None and list(p)[:5] == ["model", "image", "text", "history", "generation_config"]
    assert "session" not in inspect.signature(visualcla.VisualCLAModel.generate_many).parameters       # a follow-up


def test_session_symbols_and_constants():
    from visualcla import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "visualcla_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(vcla_\w+)\s*\(", header))
    for name in ("vcla_attn_extend", "vcla_attn_extend_scratch_bytes", "vcla_llama_extend", "vcla_llama_extend_workspace_bytes"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.vcla_version() == 5
    assert _lib.EXTEND_MAX_ROWS == int(re.search(r"#define\s+VCLA_EXTEND_MAX_ROWS\s+(\d+)", header).group(1))
    assert _lib.EXTEND_QTILE_ROWS == int(re.search(r"#define\s+VCLA_EXTEND_QTILE_ROWS\s+(\d+)", header).group(1))
    # the scratch plan is host arithmetic: one split needs none; a short block over a long cache is cut into several; more rows, more q-tiles
    sb = lib.vcla_attn_extend_scratch_bytes
    assert sb(16, 32, 128, 0) == 0 and sb(1, 32, 128, 40) == 0
    assert sb(24, 32, 128, 1900) == 32 * 15 * 64 * 132 * 4                      # H x splits (two of the 31 key tiles each) x rows of the q-tile x (d + m, l, pad) floats
    assert sb(200, 32, 128, 1000) == 32 * 2 * 8 * 128 * 132 * 4                 # two q-tiles of 128 rows, 8 splits each
    assert sb(0, 32, 128, 10) == 0 and sb(_lib.EXTEND_MAX_ROWS + 1, 32, 128, 10) == 0
    assert sb(24, 32, 128, 1900) >= sb(24, 32, 128, 600) >= sb(24, 32, 128, 200) > 0 == sb(24, 32, 128, 100)

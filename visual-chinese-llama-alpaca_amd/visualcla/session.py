"""Chat sessions: one conversation's K/V rows kept between generate() calls.

The reference's chat() (models/visualcla/modeling_utils.py:144-178) sends the whole history through model.generate on every turn; a
session is a CACHE in front of that, not another protocol: the caller still passes the full prompt, and generate(session=s) computes
only the rows behind the longest common prefix of the prompt and the ids whose rows the session holds.  The planning and recording rules
are pure functions of host lists (tests/test_session_host.py); the device side is VisualCLAModel._generate_on_stream.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch


def plan_reuse(session_ids: Sequence[int], session_image_key, new_ids: Sequence[int], slot_span: Optional[Tuple[int, int]],
               image_key) -> Tuple[int, bool]:
    """-> (P, vision_skipped).  P = number of leading rows of the session's cache the new prompt reuses: the length of the common prefix of
    `new_ids` and `session_ids`, capped at len(new_ids) - 1 (one row must run to produce logits); 0 when the prompt's image is not the
    session's (keys compared with ==; None = no image).  vision_skipped: the prompt has an image whose whole slot `slot_span` = [first, last
    + 1) of the image-token positions lies inside the reused rows, so its embeddings are not needed."""
    T = len(new_ids)
    P = 0
    if session_image_key == image_key:
        n = min(len(session_ids), T)
        while P < n and session_ids[P] == new_ids[P]:
            P += 1
    P = max(0, min(P, T - 1))
    skipped = image_key is not None and slot_span is not None and slot_span[1] <= P
    return P, skipped


def record_ids(prompt_ids: Sequence[int], returned: Sequence[int]) -> List[int]:
    """the ids whose rows the cache holds after a call: the prompt, then every returned token but the last -- that one was selected and
    never fed, so it has no row.  `returned` ends at the first eos (generate() cuts there): rows the device loop wrote behind an eos inside
    a chunk of steps belong to no recorded id and are overwritten by the next call."""
    return list(prompt_ids) + list(returned[:-1])


def image_slot_span(ids: Sequence[int], img_token_id: Optional[int]) -> Optional[Tuple[int, int]]:
    """[first, last + 1) of the positions holding the image placeholder id, None when there is none"""
    if img_token_id is None:
        return None
    pos = [i for i, t in enumerate(ids) if t == img_token_id]
    return (pos[0], pos[-1] + 1) if pos else None


def session_conflicts(gc, batch: int, image_at_head: bool, kv_fp8: bool) -> List[str]:
    """every setting of a request that a session cannot serve, by name (needs no device)"""
    bad = []
    if batch != 1:
        bad.append(f"batch size {batch} (a session is one conversation)")
    if int(getattr(gc, "num_beams", None) or 1) > 1:
        bad.append(f"num_beams={gc.num_beams}")
    if int(getattr(gc, "num_return_sequences", None) or 1) != 1:
        bad.append(f"num_return_sequences={gc.num_return_sequences}")
    if getattr(gc, "prompt_lookup_num_tokens", None) is not None:
        bad.append(f"prompt_lookup_num_tokens={gc.prompt_lookup_num_tokens}")
    if image_at_head:
        bad.append("image_at_head=True")
    if kv_fp8:
        bad.append("the e4m3 K/V cache (enable_fp8_decode(kv_cache=True))")
    return bad


class Session:
    """The K/V rows of one conversation with `model`, in a tensor of its own [layers, 2, 1, heads, capacity, head_dim] that generate()
    prefills and decodes in directly (no copy in or out).  `capacity` is fixed here because the cache layout has it as a stride:
    max_tokens, default max_position_embeddings -- 1 GiB at the 7B shape in bf16 (`nbytes`)."""

    def __init__(self, model, max_tokens: Optional[int] = None):
        t = model.config.text_config
        cap = int(max_tokens) if max_tokens is not None else int(t["max_position_embeddings"])
        if not 2 <= cap <= t["max_position_embeddings"]:
            raise ValueError(f"max_tokens must be in 2..max_position_embeddings={t['max_position_embeddings']} (got {max_tokens!r})")
        self.model = model
        self.capacity = cap
        self.kv: Optional[torch.Tensor] = None
        self._epoch = None
        self.reset()
        self._ensure()

    def reset(self) -> None:
        """forget the conversation (the buffer is kept)"""
        self.ids: List[int] = []
        self.image_key = None
        self.image: Optional[torch.Tensor] = None       # the pixel values the rows were computed from, as the vision stack saw them
        self._keys = getattr(self, "_keys", 0)

    @property
    def length(self) -> int:
        return len(self.ids)

    @property
    def nbytes(self) -> int:
        return 0 if self.kv is None else self.kv.numel() * self.kv.element_size()

    def _ensure(self) -> None:
        """the buffer, in the model's current dtype; a model rebuilt since the rows were written (dtype, fp8 switches, image size) empties
        the session"""
        m = self.model
        if self._epoch != m._session_epoch or self.kv is None or self.kv.dtype != m._dtype:
            t = m.config.text_config
            H = t["num_attention_heads"]
            self.kv = torch.empty(t["num_hidden_layers"], 2, 1, H, self.capacity, t["hidden_size"] // H, dtype=m._dtype, device=m._device)
            self._epoch = m._session_epoch
            self.reset()

    def _key_for(self, px: Optional[torch.Tensor]):
        """the session's image key when `px` (device, model dtype) holds the very values its rows were computed from, else a new key.  The
        comparison is by value, on the device."""
        if px is None:
            return None
        if self.image is not None and self.image.shape == px.shape and (px is self.image or bool(torch.equal(px, self.image))):
            return self.image_key
        self._keys += 1
        return self._keys

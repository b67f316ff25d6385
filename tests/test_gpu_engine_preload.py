"""The register preloads of the persistent B = 1 decode step (csrc/decode_engine.hip: EG_PRE / EG_PRE_O / EG_PRE_GU slots per consumer wave, taken
unconditionally) at the edge of the geometry guard `upc, gpc, s_lm >= 2 * EG_PRE_MAX` (vcla_engine_geometry and its mirror weights.engine_geometry):
two layers at the engine's fixed width (hidden 4096), the smallest operators the guard admits, and one size below each bound.

Sizes.  gpc = ceil(upc / 2) >= 8 is the binding bound on the MLP, so the smallest admissible intermediate sizes are 256 * 15 (odd upc: the single last
SwiGLU unit, gpc = 8) and 256 * 16 (even, gpc = 8): gate/up is then 8 preloaded + 7 or 8 shared slots per CU, down_proj 3 preloaded + 5.  (256 * 2 *
EG_PRE_MAX = 2048 would make gate/up consist of preloaded slots only, but gives gpc = 4, which the guard refuses.)  The vocabulary is exactly
2 * EG_PRE_MAX * 512 = 4096 rows: s_lm = 8, no ragged last slot.  One below: upc = 14 (gpc = 7), and 4096 - 512 rows (s_lm = 7).

Bounds: those tests/test_gpu_engine.py states for its 3-layer model (logits 0.2 max / 0.04 mean, appended K / V rows 0.15); this model has 2 layers."""
import os

import pytest
import torch

from tests.test_gpu_engine import _Prefilled, _steps

pytestmark = pytest.mark.gpu

EG_PRE_MAX = 4
V_MIN = 2 * EG_PRE_MAX * 512                    # s_lm = 8
I_EVEN, I_ODD = 256 * 4 * EG_PRE_MAX, 256 * (4 * EG_PRE_MAX - 1)       # upc 16 / 15, gpc 8
I_BELOW, V_BELOW = 256 * (4 * EG_PRE_MAX - 2), V_MIN - 512             # gpc 7; s_lm 7

_models = {}


def _model(inter, vocab):
    """one model per geometry, built once and shared by the tests of this file"""
    if (inter, vocab) not in _models:
        import visualcla
        cfg = visualcla.visualcla_7b_config()
        cfg.text_config.update(num_hidden_layers=2, vocab_size=vocab, intermediate_size=inter)
        cfg.vision_config.update(num_hidden_layers=1, hidden_size=256, intermediate_size=512, num_attention_heads=4)
        cfg.visual_resampler_config.update(num_hidden_layers=1, hidden_size=256, intermediate_size=512, num_attention_heads=4)
        _models[(inter, vocab)] = visualcla.VisualCLAModel.from_random(cfg, device="cuda:0", torch_dtype=torch.bfloat16, seed=3)
    return _models[(inter, vocab)]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    os.environ.pop("VCLA_ENGINE", None)
    _models.clear()
    torch.cuda.empty_cache()


def test_the_guard_admits_exactly_these_sizes():
    from visualcla.weights import engine_geometry
    for inter in (I_EVEN, I_ODD):
        g = engine_geometry(4096, 32, inter, V_MIN, 2)
        assert g is not None and g["gpc"] == 2 * EG_PRE_MAX and g["s_lm"] == 2 * EG_PRE_MAX and g["upc"] == inter // 256
    assert engine_geometry(4096, 32, I_BELOW, V_MIN, 2) is None
    assert engine_geometry(4096, 32, I_EVEN, V_BELOW, 2) is None


@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("inter", [I_EVEN, I_ODD])
def test_smallest_geometry_matches_the_launch_path(inter, T):
    """every operator at its smallest: 3 decode steps, teacher-forced on the launch path's tokens"""
    m = _model(inter, V_MIN)
    assert "llama.engine.w" in m._packed
    n = 3
    try:
        label = _Prefilled(m, T, False).step("1", T, torch.tensor([17], device=m.device))[1]
        assert label.startswith("decode_engine_kernel"), label
        t0, l0, kv0 = _steps(m, "0", T, n, False)
        t1, l1, kv1 = _steps(m, "1", T, n, False, forced=t0)
    finally:
        os.environ.pop("VCLA_ENGINE", None)
    for s in range(n):
        d = (l0[s] - l1[s]).abs()
        print(f"[engine_preload] inter={inter} T={T} step {s}: engine vs launch path max {d.max().item():.4f} mean {d.mean().item():.5f}")
        assert torch.isfinite(l1[s]).all()
        assert d.max().item() <= 0.2 and d.mean().item() <= 0.04, (inter, T, s, d.max().item(), d.mean().item())
        top2 = l0[s].topk(2, dim=-1).values[0]
        if float(top2[0] - top2[1]) > 0.3:
            assert int(l0[s].argmax()) == int(l1[s].argmax()), (inter, T, s)
    assert (kv0[..., T:, :] - kv1[..., T:, :]).abs().max().item() <= 0.15
    assert (kv1[..., T:, :].abs().amax(dim=(-1,)) > 0).all()


@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("inter", [I_EVEN, I_ODD])
def test_smallest_geometry_graph_loop_equals_eager_loop(inter, T):
    """the hipGraph replay of one captured engine step against eager launches: token for token"""
    m = _model(inter, V_MIN)
    os.environ["VCLA_ENGINE"] = "1"
    try:
        ids = torch.randint(3, V_MIN - 8, (1, T), generator=torch.Generator().manual_seed(9)).to(m.device)
        kw = dict(input_ids=ids, max_new_tokens=4, do_sample=False, eos_token_id=None)       # the prefill's token + 3 decode steps
        a = m.generate(use_graph=True, **kw)
        b = m.generate(use_graph=False, **kw)
    finally:
        os.environ.pop("VCLA_ENGINE", None)
    assert a.shape == (1, 4) and torch.equal(a, b), (a.tolist(), b.tolist())


@pytest.mark.parametrize("inter,vocab", [(I_BELOW, V_MIN), (I_EVEN, V_BELOW)])
def test_one_size_below_a_bound_is_served_by_the_launch_path(inter, vocab):
    """an operator one slot short of the unconditional preloads: no engine stream, the launch path whatever VCLA_ENGINE says, bit-equal results"""
    m = _model(inter, vocab)
    assert "llama.engine.w" not in m._packed
    T, n = 37, 3
    try:
        label = _Prefilled(m, T, False).step("1", T, torch.tensor([17], device=m.device))[1]
        assert not label.startswith("decode_engine_kernel"), label
        t0, l0, kv0 = _steps(m, "0", T, n, False)
        t1, l1, kv1 = _steps(m, "1", T, n, False)
    finally:
        os.environ.pop("VCLA_ENGINE", None)
    assert t0 == t1
    for s in range(n):
        assert torch.equal(l0[s], l1[s]), s
    assert torch.equal(kv0, kv1)

"""Every VCLA_* A/B switch the product library reads (csrc/vcla_knobs.h) selects a kernel form that was the default at
some point: each must still produce the reference's numbers.  One child process per setting: small model, bf16, forward logits within the
bf16 bound of the fp32 oracle and greedy ids equal wherever the oracle's margin allows.  The library reads the switches at every outermost
call; test_switch_flip_in_process_recaptures_the_graphs checks that a flip inside one process reaches the cached graphs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = [
    {},                                     # defaults
    {"VCLA_DSTREAM": "0"},                  # split-K panel kernels instead of the streaming decode GEMMs
    {"VCLA_DS_DEFER": "0"},                 # a norm launch per RMSNorm instead of the deferred form
    {"VCLA_DS_QKV_SPLIT": "0"},             # qkv unsplit + plain decode attention instead of two raw K slices summed by the attention kernel
    {"VCLA_GEMV1X": "0"},                   # runtime-K decode GEMV
    {"VCLA_ATTN_MFMA_WHOLE": "0"},
    {"VCLA_GEMM_PF": "0"},                  # the 256 x 256 GEMM without the L2 prefetch (and without 257-row tiles)
    {"VCLA_GEMM_XR": "0"},                  # 256-row tiles + a tail launch for the ViT's M = B * 257
    {"VCLA_MFMA128_SPLITK": "0"},
    {"VCLA_MACRO_GRAPH": "0"},
    {"VCLA_DECODE_GRAPH": "0"},
]


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "defaults")
def test_env_switch_keeps_parity(env):
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("VCLA_") or k == "VCLA_LIB"}
    child_env.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "env_switch_child.py")], env=child_env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    for tag, v in res.items():
        assert v["max"] <= 6e-2 and v["mean"] <= 1e-2 and v["ids_agree"], (env, tag, v)


MACRO_CHILD = r"""
import os, sys, torch
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "visual-chinese-llama-alpaca_amd")):
    sys.path.insert(0, p)
from oracle import visualcla_oracle as O
from tests.helpers import make_hip_model
cfg = O.cfg_small()
W = O.make_weights(cfg, seed=0)
m = make_hip_model(cfg, W, torch.bfloat16)
reqs = [tuple(t.cuda() if i else t.cuda().to(torch.bfloat16) for i, t in enumerate(O.make_inputs(cfg, B, 48))) for B in (3, 2)]   # resident request buffers (the graph key holds their addresses)
first = {}
for i in range(10):                      # two request shapes in strict alternation
    px, ids, mask = reqs[i % 2]
    t = m.generate(input_ids=ids, pixel_values=px, attention_mask=mask, max_new_tokens=4, do_sample=False, eos_token_id=None).cpu()
    assert i % 2 not in first or torch.equal(t, first[i % 2]), i
    first.setdefault(i % 2, t)
    print(f"CALL {i}", file=sys.stderr, flush=True)
print("MACRO_OK")
"""


def test_macro_graphs_keep_two_shapes_cached(tmp_path):
    """the vision-stack / prefill graph cache holds TWO keys: a caller alternating between two request shapes (A, B, A, B, ...) replays both
    after the warm-up instead of re-running eager + capture on every other call; results stay identical call to call"""
    script = tmp_path / "macro_child.py"
    script.write_text(MACRO_CHILD)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VCLA_") or k == "VCLA_LIB"}
    env["VCLA_MACRO_GRAPH_DEBUG"] = "1"
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "MACRO_OK" in r.stdout, r.stderr[-3000:]
    calls = r.stderr.split("CALL ")
    # each generate() = one vision-graph and one prefill-graph decision; from the 5th call on (A and B both seen twice) every decision is a replay
    for i, chunk in enumerate(calls[:-1]):
        lines = [ln for ln in chunk.splitlines() if "macro graph" in ln]
        if i >= 4:
            assert lines and all("replay" in ln for ln in lines), (i, lines)


FLIP_CHILD = r"""
import os, sys, torch
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "visual-chinese-llama-alpaca_amd")):
    sys.path.insert(0, p)
from oracle import visualcla_oracle as O
from tests.helpers import cfg_engine_small, make_hip_model
cfg = cfg_engine_small()
W = O.make_weights(cfg, seed=1)
m = make_hip_model(cfg, W, torch.bfloat16)
assert "llama.engine.w" in m._packed
px, ids, mask = (t.cuda() if i else t.cuda().to(torch.bfloat16) for i, t in enumerate(O.make_inputs(cfg, 1, 24)))   # resident request buffers
toks = []
for i in range(3):
    if i == 2:       # same forms at this geometry (contexts < 512, no ring-tile ViT shape), other switch values: the cached graphs must not be replayed
        os.environ["VCLA_ENGINE_SPLIT"] = "0"
        os.environ["VCLA_RING_VIT"] = "0"
    print(f"CALL {i}", file=sys.stderr, flush=True)
    toks.append(m.generate(input_ids=ids, pixel_values=px, attention_mask=mask, max_new_tokens=6, do_sample=False, eos_token_id=None).cpu())
    torch.cuda.synchronize()
assert all(torch.equal(t, toks[0]) for t in toks), [t.tolist() for t in toks]
print("FLIP_OK")
"""


def test_switch_flip_in_process_recaptures_the_graphs(tmp_path):
    """the switches are read at every outermost call and the snapshot is part of every graph key: generate() twice (B = 1, the persistent decode
    step; the second call replays the vision, prefill and decode graphs), then VCLA_ENGINE_SPLIT and VCLA_RING_VIT change inside the process --
    the next call runs the macro graphs eagerly on a new key and captures the decode graph again instead of replaying graphs chosen under the old
    values; the tokens stay the same"""
    script = tmp_path / "flip_child.py"
    script.write_text(FLIP_CHILD)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VCLA_") or k == "VCLA_LIB"}
    env["VCLA_MACRO_GRAPH_DEBUG"] = "1"
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FLIP_OK" in r.stdout, r.stderr[-3000:]
    calls = r.stderr.split("CALL ")[1:]
    assert len(calls) == 3, r.stderr[-3000:]
    macro = [[ln for ln in c.splitlines() if "macro graph" in ln] for c in calls]
    decode = [[ln for ln in c.splitlines() if "decode graph" in ln] for c in calls]
    assert macro[1] and all("replay" in ln for ln in macro[1]), macro[1]
    assert decode[1] and all("replay" in ln for ln in decode[1]), decode[1]
    assert macro[2] and not any("replay" in ln for ln in macro[2]), macro[2]
    assert decode[2] and any("capture" in ln for ln in decode[2]) and not any("replay" in ln for ln in decode[2]), decode[2]


VIT_CHILD = r"""
import math, os, sys, torch
ROOT = sys.argv[1]
for p in (ROOT, os.path.join(ROOT, "visual-chinese-llama-alpaca_amd")):
    sys.path.insert(0, p)
from visualcla import _lib
B, H, T, D = 9, 16, 257, 64
g = torch.Generator().manual_seed(5)
q, k, v = (torch.randn(B, H, T, D, generator=g).to(torch.bfloat16) for _ in range(3))
s = (q.float() @ k.float().transpose(-1, -2)) / math.sqrt(D)
ref = (torch.softmax(s, -1) @ v.float()).transpose(1, 2).reshape(B, T, H * D)
out = torch.empty(B, T, H * D, dtype=torch.bfloat16, device="cuda:0")
for fk in (3, 0):          # forced, and the automatic dispatch (B * H = 144 >= 128)
    out.fill_(7.0)
    _lib.attention(q.cuda(), k.cuda(), v.cuda(), 1 / math.sqrt(D), causal=False, out=out, force_kernel=fk)
    torch.cuda.synchronize()
    err = (out.float().cpu() - ref).abs().max().item()
    assert err <= 2e-2, (fk, err)
print("VIT_OK")
"""


@pytest.mark.parametrize("form", ["0", "1", "2"])
def test_vit_attention_forms_by_env(tmp_path, form):
    """VCLA_ATTN_VIT = 0 (tile-by-tile kernel), 1 (register-staged whole-sequence form), 2 (direct-to-LDS pipelined form, the default): each
    against the fp32 reference on a 257-token ViT shape, forced and through the automatic dispatch"""
    script = tmp_path / "vit_child.py"
    script.write_text(VIT_CHILD)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VCLA_") or k == "VCLA_LIB"}
    env["VCLA_ATTN_VIT"] = form
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "VIT_OK" in r.stdout, r.stderr[-2000:]

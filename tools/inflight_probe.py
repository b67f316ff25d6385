"""In-flight batching at the full 7B shape (synthetic weights as bench.py builds them, bf16): what a slots step costs next to the uniform
decode step, and what generate_many buys on a queue of requests with very different lengths against generate() on consecutive batches.

    python tools/inflight_probe.py [--requests 256] [--slots 64] [--prompt 128] [--steps-per-sync 8] [--seed 0] [--out profiles/inflight_batching.txt]

The parent process never touches the GPU: it prints the step-count prediction (host arithmetic, visualcla/inflight.py), then runs every
GPU leg as a child process under a time limit of its own and stops at the first leg that fails.  Every leg prints one JSON line; the parent
writes them to --out.

    step_cost   ms per step of vcla_llama_decode_slots (all slots active at equal positions) against vcla_llama_decode_loop at the same batch
                and context in the same process, both with a key mask of ones, alternating; the unmasked uniform loop for information
    queue       useful tokens/s of generate_many over the queue against generate() on consecutive groups of `slots` requests run to each
                group's largest budget (eos off, one image per request, budgeted tokens only)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "visual-chinese-llama-alpaca_amd"))

import numpy as np  # noqa: E402


def budgets_of(seed: int, n: int):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(np.exp(rng.normal(np.log(96), 0.8, n))), 8, 512).astype(int).tolist()


def prediction(args) -> dict:
    from visualcla import inflight as I
    b = budgets_of(args.seed, args.requests)
    sch, _ = I.simulate(b, args.slots, args.steps_per_sync)
    static = I.static_batch_steps(b, args.slots)
    return {"leg": "prediction", "requests": args.requests, "slots": args.slots, "steps_per_sync": args.steps_per_sync, "budget_mean": round(float(np.mean(b)), 1),
            "budget_max": max(b), "budgeted_tokens": sum(b), "static_steps": static, "inflight_steps": sch.stats["steps"],
            "ideal_steps": -(-sum(x - 1 for x in b) // args.slots), "step_bound": round(I.step_bound(b, args.slots, args.steps_per_sync), 1),
            "predicted_decode_ratio": round(static / max(sch.stats["steps"], 1), 3)}


def _model(args):
    import torch
    import visualcla
    from visualcla import _lib
    from visualcla.synthetic import stub_tokenizer
    _lib.require_device()                                        # no GPU: fail here, loudly
    cfg = visualcla.visualcla_7b_config()
    if args.layers:
        cfg.text_config["num_hidden_layers"] = args.layers
    model = visualcla.VisualCLAModel.from_random(cfg, device=torch.device("cuda", 0), torch_dtype=torch.bfloat16, seed=0)
    model.tokenizer = stub_tokenizer()
    model.image_at_head = False
    return model


def leg_step_cost(args) -> dict:
    import torch
    from visualcla import _lib
    model = _model(args)
    lib = _lib.load()
    dev = model.device
    t = model.config.text_config
    B, T, n = args.slots, args.prompt, args.steps
    ctx_max = (T + n + 2 + 63) // 64 * 64
    H, d = t["num_attention_heads"], t["hidden_size"] // t["num_attention_heads"]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        kv = (torch.randn(t["num_hidden_layers"], 2, B, H, ctx_max, d, device=dev) * 0.3).to(torch.bfloat16)
        km = torch.ones(B, ctx_max, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.vcla_llama_workspace_bytes(model._ctx, B, 1) + 512, dtype=torch.uint8, device=dev)
        ids = torch.randint(3, t["vocab_size"] - 8, (B,), generator=torch.Generator().manual_seed(3)).to(dev)
        out = torch.zeros(n, B, dtype=torch.int64, device=dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        W = _lib.SLOT_SUMMARY_WORDS
        st = torch.zeros(4 * B + W, dtype=torch.int32, device=dev)
        hist = torch.zeros(n + 2, B, dtype=torch.int64, device=dev)
        cur = ids.clone()
        slots = _lib.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
        init = torch.tensor([T] * B + [1] * B + [1] * B + [n + 2] * B + [0] * W, dtype=torch.int32, device=dev)

        def uniform(mask, steps):
            pos_dev.zero_()
            _lib.check(lib.vcla_llama_decode_loop(model._ctx, ids.data_ptr(), B, T, pos_dev.data_ptr(), steps, kv.data_ptr(), ctx_max, _lib.ptr(mask), out.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), 1, _lib.stream_ptr()))

        def slotted(steps):
            st.copy_(init)
            cur.copy_(ids)
            _lib.check(lib.vcla_llama_decode_slots(model._ctx, C.byref(slots), steps, kv.data_ptr(), ctx_max, km.data_ptr(), ws.data_ptr(), ws.numel(), 1, None,
                                                   _lib.stream_ptr()))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        legs = {"uniform_masked": lambda: uniform(km, n), "slots": lambda: slotted(n), "uniform_unmasked": lambda: uniform(None, n)}
        for fn in (lambda: uniform(km, 8), lambda: slotted(8), lambda: uniform(None, 8)):      # warm-up: code objects, the three graphs
            fn()
        torch.cuda.synchronize()
        assert st[4 * B].item() == B, "every slot must still be active"
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):                             # alternating
            for k, fn in legs.items():
                ms[k].append(timed(fn))
        assert st[4 * B].item() == B and st[:B].tolist() == [T + n] * B
    best = {k: min(v) for k, v in ms.items()}
    return {"leg": "step_cost", "B": B, "context": f"{T}..{T + n}", "steps_per_sample": n, "samples_each": args.rounds,
            "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "ms_per_step_min": {k: round(v, 4) for k, v in best.items()},
            "slots_over_uniform_masked": round(best["slots"] / best["uniform_masked"], 4), "margin": "slots step at most 1.05 x the uniform step of the same run"}


def leg_queue(args) -> dict:
    import torch
    from visualcla.synthetic import make_inputs
    model = _model(args)
    B, T, N = args.slots, args.prompt, args.requests
    b = budgets_of(args.seed, N)
    px, ids, _ = make_inputs(model.config, N, T)
    px, ids = px.to(model.device, torch.bfloat16), ids.to(model.device)
    reqs = [dict(input_ids=ids[i], pixel_values=px[i], max_new_tokens=b[i]) for i in range(N)]
    kw = dict(do_sample=False, eos_token_id=None)

    def static():
        outs = []
        for i in range(0, N, B):
            o = model.generate(input_ids=ids[i:i + B], pixel_values=px[i:i + B], max_new_tokens=max(b[i:i + B]), **kw)
            outs.append(o)
        torch.cuda.synchronize()
        return outs

    def inflight():
        o = model.generate_many(reqs, max_batch=B, steps_per_sync=args.steps_per_sync, **kw)
        torch.cuda.synchronize()
        return o
    # warm-up: every shape of the timed windows once (code objects, graphs): one short lock-step batch, one short queue
    model.generate(input_ids=ids[:B], pixel_values=px[:B], max_new_tokens=9, **kw)
    model.generate_many([dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])], max_batch=B, steps_per_sync=args.steps_per_sync, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    static()
    t_static = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = inflight()
    t_inflight = time.perf_counter() - t0
    st = dict(model.last_inflight_stats)
    assert [len(x) for x in got] == b
    useful = sum(b)
    return {"leg": "queue", "requests": N, "slots": B, "prompt": T, "budgeted_tokens": useful, "static_s": round(t_static, 3), "inflight_s": round(t_inflight, 3),
            "static_tok_s": round(useful / t_static, 1), "inflight_tok_s": round(useful / t_inflight, 1), "speedup": round(t_static / t_inflight, 3),
            "admission_groups": st["admission_groups"], "admission_s": round(st["admission_s"], 3), "steps_s": round(st["steps_s"], 3), "steps": st["steps"],
            "slot_occupancy": round(st["slot_steps_active"] / max(st["slot_steps_total"], 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps-per-sync", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100, help="step_cost: steps per timed sample")
    ap.add_argument("--rounds", type=int, default=3, help="step_cost: alternating samples per loop")
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--leg", choices=["step_cost", "queue"], help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "inflight_batching.txt"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps({"step_cost": leg_step_cost, "queue": leg_queue}[args.leg](args)), flush=True)
        return 0
    lines = [json.dumps(prediction(args))]
    print(lines[0], flush=True)
    if args.predict_only:
        return 0
    for leg in ("step_cost", "queue"):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg] + \
              [x for k in ("requests", "slots", "prompt", "steps_per_sync", "seed", "steps", "rounds", "layers") for x in (f"--{k.replace('_', '-')}", str(getattr(args, k)))]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                    # nothing more is started on the GPU after a failed leg
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"inflight_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/inflight_probe.py on MI355X: one JSON line per leg (prediction: host arithmetic; step_cost, queue: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Per-request generation configs at the full 7B shape (synthetic weights as bench.py builds them, bf16): what the slots step costs when every
row reads its sampler parameters from a record in device memory, and what one mixed generate_many call buys over one call per config.

    python tools/per_request_probe.py [--requests 256] [--slots 64] [--prompt 128] [--steps-per-sync 8] [--seed 0] [--out profiles/per_request_sampling.txt]

The parent process never touches the GPU: it prints the step-count prediction (host arithmetic, visualcla/inflight.py), then runs every
GPU leg as a child process under a time limit of its own and stops at the first leg that fails.  Every leg prints one JSON line; the parent
writes them to --out.

    step_cost   ms per graph-replayed slots step at B = slots, all slots active: (a) argmax, (b) the sampler with one parameter block for all
                rows (vcla_llama_decode_slots), (c) the sampler with `slots` DISTINCT records and the per-row eos table
                (vcla_llama_decode_slots_rows); alternating in one process, `--rounds` takes each.  Condition: (c) is no slower than (b) beyond
                the spread the takes of (b) show, and never beyond 1.05 x (the margin of DESIGN.md section 7e)
    queue       the inflight_probe queue under four config classes (request i is of class i % 4: greedy; the reference's default sampling
                config; top_k = 1 with penalties; temperature 1.0, top_p 0.95, top_k 50): useful tokens/s of ONE mixed call against four
                uniform calls of requests/4 requests each, which is how such a queue is served without per-request configs
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from inflight_probe import _model, budgets_of  # noqa: E402

PARENT_SLOTS_STEP_MS = 4.539      # profiles/inflight_batching.txt, step_cost: the argmax slots step before the per-slot tables existed

CLASSES = [
    dict(do_sample=False),
    dict(do_sample=True, temperature=0.5, top_k=40, top_p=0.9, repetition_penalty=1.1, no_repeat_ngram_size=15),      # models/visualcla/modeling_utils.py:36-47
    dict(do_sample=True, top_k=1, repetition_penalty=1.1, no_repeat_ngram_size=3),
    dict(do_sample=True, temperature=1.0, top_p=0.95, top_k=50),
]


def prediction(args) -> dict:
    from visualcla import inflight as I
    b = budgets_of(args.seed, args.requests)
    mixed, _ = I.simulate(b, args.slots, args.steps_per_sync)
    split = [I.simulate(b[c::4], args.slots, args.steps_per_sync)[0].stats["steps"] for c in range(4)]
    return {"leg": "prediction", "requests": args.requests, "slots": args.slots, "steps_per_sync": args.steps_per_sync, "budgeted_tokens": sum(b),
            "budgeted_tokens_per_class": [sum(b[c::4]) for c in range(4)], "mixed_steps": mixed.stats["steps"], "split_steps": split,
            "predicted_decode_ratio": round(sum(split) / max(mixed.stats["steps"], 1), 3)}


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
        W = _lib.SLOT_SUMMARY_WORDS
        st = torch.zeros(4 * B + W, dtype=torch.int32, device=dev)
        hist = torch.zeros(n + 2, B, dtype=torch.int64, device=dev)
        uni = torch.rand(n + 2, B, device=dev)
        cur = ids.clone()
        slots = _lib.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
        init = torch.tensor([T] * B + [1] * B + [1] * B + [n + 2] * B + [0] * W, dtype=torch.int32, device=dev)
        base = dict(repetition_penalty=1.1, no_repeat_ngram_size=15, temperature=0.5, top_k=40, top_p=0.9)
        samp = _lib.sample_args(uniforms=uni, history=hist, **base)
        shared = _lib.sample_args(uniforms=uni, history=hist)
        # B distinct records around the reference default: no two rows share temperature, top_p or repetition_penalty.  top_k stays at (b)'s
        # 40: it sets the sampler's WORK (bisection passes, the size of the rank sort), and a launch lasts as long as its slowest row --
        # the comparison is about where the parameters come from, not about which parameters they are
        records = [dict(base, temperature=0.4 + 0.005 * b, top_p=0.85 + 0.002 * b, repetition_penalty=1.05 + 0.002 * b) for b in range(B)]
        assert len({tuple(sorted(r.items())) for r in records}) == B
        rows = _lib.sample_row_bytes(_lib.sample_row_table(records)).to(dev)
        eos_rows = _lib.slot_eos_rows([[]] * B).to(dev)

        def run(which, steps):
            st.copy_(init)
            cur.copy_(ids)
            head = (model._ctx, C.byref(slots), steps, kv.data_ptr(), ctx_max, km.data_ptr(), ws.data_ptr(), ws.numel(), 1)
            if which == "argmax":
                _lib.check(lib.vcla_llama_decode_slots(*head, None, _lib.stream_ptr()))
            elif which == "uniform_sampler":
                _lib.check(lib.vcla_llama_decode_slots(*head, C.byref(samp), _lib.stream_ptr()))
            else:
                _lib.check(lib.vcla_llama_decode_slots_rows(*head, C.byref(shared), eos_rows.data_ptr(), rows.data_ptr(), _lib.stream_ptr()))

        def timed(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run(which, 1)                                        # one graph slot, three alternating keys: the capture happens here, untimed
            e0.record(stream)
            run(which, n)
            e1.record(stream)
            torch.cuda.synchronize()
            assert st[4 * B].item() == B and st[:B].tolist() == [T + n] * B, "every slot must still be active"
            return e0.elapsed_time(e1) / n
        names = ("argmax", "uniform_sampler", "table")
        for k in names:                                          # warm-up: code objects
            run(k, 8)
        torch.cuda.synchronize()
        ms = {k: [] for k in names}
        for _ in range(args.rounds):                             # alternating
            for k in names:
                ms[k].append(timed(k))
    best = {k: min(v) for k, v in ms.items()}
    spread_b = max(ms["uniform_sampler"]) - min(ms["uniform_sampler"])
    ok = best["table"] <= best["uniform_sampler"] + spread_b and best["table"] <= 1.05 * best["uniform_sampler"]
    return {"leg": "step_cost", "B": B, "context": f"{T}..{T + n}", "steps_per_sample": n, "samples_each": args.rounds,
            "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "ms_per_step_min": {k: round(v, 4) for k, v in best.items()},
            "spread_uniform_sampler_ms": round(spread_b, 4), "table_over_uniform_sampler": round(best["table"] / best["uniform_sampler"], 4),
            "condition": "table <= uniform_sampler + spread of uniform_sampler's takes, and <= 1.05 x uniform_sampler", "condition_met": bool(ok),
            "argmax_over_parent_slots_step": round(best["argmax"] / PARENT_SLOTS_STEP_MS, 4), "parent_slots_step_ms": PARENT_SLOTS_STEP_MS,
            "note": "table: 64 records that differ in temperature, top_p and repetition_penalty at the uniform variant's top_k; every timed window replays a captured step"}


def leg_queue(args) -> dict:
    import torch
    from visualcla.synthetic import make_inputs
    model = _model(args)
    B, T, N = args.slots, args.prompt, args.requests
    b = budgets_of(args.seed, N)
    px, ids, _ = make_inputs(model.config, N, T)
    px, ids = px.to(model.device, torch.bfloat16), ids.to(model.device)
    reqs = [dict(input_ids=ids[i], pixel_values=px[i], max_new_tokens=b[i]) for i in range(N)]
    queue_kw = dict(do_sample=False, eos_token_id=None)

    def mixed(rs, first=0):
        o = model.generate_many([dict(r, generation_config=CLASSES[(first + k) % 4], seed=first + k) for k, r in enumerate(rs)], max_batch=B,
                                steps_per_sync=args.steps_per_sync, **queue_kw)
        torch.cuda.synchronize()
        return o

    def split(rs_of):
        outs = []
        for c in range(4):
            outs.append(model.generate_many([dict(r, seed=i) for i, r in rs_of(c)], max_batch=B, steps_per_sync=args.steps_per_sync, eos_token_id=None, **CLASSES[c]))
        torch.cuda.synchronize()
        return outs
    # warm-up: every route of the timed windows once on a short queue (code objects, graphs)
    short = [dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])]
    mixed(short)
    split(lambda c: list(enumerate(short))[c::4])
    torch.cuda.manual_seed(0)
    t0 = time.perf_counter()
    got = mixed(reqs)
    t_mixed = time.perf_counter() - t0
    st = dict(model.last_inflight_stats)
    assert [len(x) for x in got] == b and st["config_classes"] == 4
    t0 = time.perf_counter()
    parts = split(lambda c: list(enumerate(reqs))[c::4])
    t_split = time.perf_counter() - t0
    assert [len(x) for c in range(4) for x in parts[c]] == [n for c in range(4) for n in b[c::4]]
    useful = sum(b)
    return {"leg": "queue", "requests": N, "slots": B, "prompt": T, "budgeted_tokens": useful, "classes": CLASSES, "mixed_s": round(t_mixed, 3),
            "split_s": round(t_split, 3), "mixed_tok_s": round(useful / t_mixed, 1), "split_tok_s": round(useful / t_split, 1),
            "mixed_over_split": round(t_split / t_mixed, 3), "mixed_steps": st["steps"], "mixed_admission_s": round(st["admission_s"], 3),
            "mixed_steps_s": round(st["steps_s"], 3), "sampler_rows": st["sampler_rows"], "seeded": st["seeded"],
            "slot_occupancy": round(st["slot_steps_active"] / max(st["slot_steps_total"], 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps-per-sync", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100, help="step_cost: steps per timed sample")
    ap.add_argument("--rounds", type=int, default=2, help="step_cost: alternating takes per variant")
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--leg", choices=["step_cost", "queue"], help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "per_request_sampling.txt"))
    args = ap.parse_args()
    if args.requests % 4:
        ap.error("--requests must be a multiple of 4 (four config classes of equal size)")
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
            print(f"per_request_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/per_request_probe.py on MI355X: one JSON line per leg (prediction: host arithmetic; step_cost, queue: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

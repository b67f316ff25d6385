"""Stop sequences, streamed tokens and cancellation at the full 7B shape (synthetic weights as bench.py builds them, bf16): what the stop
table costs a slots step, what stopping requests early gives back on the queue of inflight_probe, and what a token callback adds to a
boundary.

    python tools/stops_probe.py [--requests 256] [--slots 64] [--prompt 128] [--steps-per-sync 8] [--seed 0] [--parent-tree DIR]
                                [--out profiles/stop_sequences.txt]

The parent process never touches the GPU: it prints the step-count prediction (host arithmetic, visualcla/inflight.py), then runs every
GPU leg as a child process under a time limit of its own and stops at the first leg that fails.  Every leg prints one JSON line; the parent
writes them to --out.

    step_cost   ms per graph-replayed slots step at B = slots, all slots active, argmax path: a null stop table (the launches and the kernel
                instantiation of the commit before stop sequences) against four 16-id sequences on every slot, none of which ever hits;
                `--rounds` takes of `--steps` steps each, alternating in one process.  --parent-tree DIR (a built checkout of the parent
                commit): its own tools/inflight_probe.py step_cost leg runs before and after ours, in the same session, and its `slots` step
                is the parent's figure.  Conditions: the step with stops at most 1.05 x the parent's; the null step within the parent's spread
    queue       the inflight_probe queue (eos off) run to its budgets, then with one 2-id stop sequence per request drawn from its own free
                run at a random point: steps, occupancy and wall time of both, beside the step count the host simulation predicts; then the
                free queue again with a no-op on_tokens callback: the time a boundary gains
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "visual-chinese-llama-alpaca_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from inflight_probe import _model, budgets_of  # noqa: E402


def _cut_points(budgets, seed):
    """request i's stop sequence ends at its p_i-th token: 2 <= p_i <= budget_i"""
    rng = random.Random(seed + 1)
    return [rng.randint(2, b) for b in budgets]


def prediction(args) -> dict:
    from visualcla import inflight as I
    b = budgets_of(args.seed, args.requests)
    p = _cut_points(b, args.seed)
    tok = lambda i, k: 1000 * (i + 1) + k                         # noqa: E731  (simulate's stream)
    free, _ = I.simulate(b, args.slots, args.steps_per_sync)
    cut, _ = I.simulate(b, args.slots, args.steps_per_sync, stops=[[[tok(i, q - 1), tok(i, q)]] for i, q in enumerate(p)])
    assert [len(x) for x in cut.ordered_results()] == p and cut.stats["stop_hits"] == len(b)
    occ = lambda s: round(s.stats["slot_steps_active"] / max(s.stats["slot_steps_total"], 1), 4)      # noqa: E731
    return {"leg": "prediction", "requests": args.requests, "slots": args.slots, "steps_per_sync": args.steps_per_sync, "budgeted_tokens": sum(b),
            "tokens_up_to_the_stops": sum(p), "free_steps": free.stats["steps"], "stopped_steps": cut.stats["steps"],
            "free_occupancy": occ(free), "stopped_occupancy": occ(cut), "predicted_step_ratio": round(cut.stats["steps"] / max(free.stats["steps"], 1), 4),
            "table_bytes": args.slots * 64 * 4,
            "note": "the stop table is 256 bytes per slot, read by one wave of the bookkeeping launch: 16 KiB per step at B = 64 against a step "
                    "that streams the 13 GB of weights"}


def leg_step_cost(args) -> dict:
    import torch
    from visualcla import _lib
    model = _model(args)
    lib = _lib.load()
    dev = model.device
    t = model.config.text_config
    B, T, n, V = args.slots, args.prompt, args.steps, t["vocab_size"]
    ctx_max = (T + n + 2 + 63) // 64 * 64
    H, d = t["num_attention_heads"], t["hidden_size"] // t["num_attention_heads"]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        kv = (torch.randn(t["num_hidden_layers"], 2, B, H, ctx_max, d, device=dev) * 0.3).to(torch.bfloat16)
        km = torch.ones(B, ctx_max, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.vcla_llama_workspace_bytes(model._ctx, B, 1) + 512, dtype=torch.uint8, device=dev)
        ids = torch.randint(3, V - 8, (B,), generator=torch.Generator().manual_seed(3)).to(dev)
        W = _lib.SLOT_SUMMARY_WORDS
        st = torch.zeros(4 * B + W, dtype=torch.int32, device=dev)
        hist = torch.zeros(n + 2, B, dtype=torch.int64, device=dev)
        cur = ids.clone()
        slots = _lib.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
        init = torch.tensor([T] * B + [1] * B + [1] * B + [n + 2] * B + [0] * W, dtype=torch.int32, device=dev)
        # four sequences of 16 ids on every slot; every lane compares (the history holds ids from step 1 on), none of them ever completes
        rng = random.Random(args.seed)
        table = _lib.slot_stop_rows([[[rng.randrange(3, V) for _ in range(15)] + [V - 1 - s] for s in range(4)] for _ in range(B)]).to(dev)
        stops = _lib.stop_args(table)

        def run(kind, steps):
            st.copy_(init)
            cur.copy_(ids)
            _lib.check(lib.vcla_llama_decode_slots_stops(model._ctx, C.byref(slots), steps, kv.data_ptr(), ctx_max, km.data_ptr(), ws.data_ptr(), ws.numel(), 1,
                                                         None, None, None, None, None, C.byref(stops) if kind == "stops4x16" else None, _lib.stream_ptr()))

        def timed(kind):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run(kind, 1)                                         # one graph slot, alternating keys: the capture happens here, untimed
            e0.record(stream)
            run(kind, n)
            e1.record(stream)
            torch.cuda.synchronize()
            assert st[4 * B].item() == B and st[:B].tolist() == [T + n] * B, "every slot must still be active"
            return e0.elapsed_time(e1) / n
        kinds = ("null", "stops4x16")
        taken = {}
        for k in kinds:                                          # warm-up: code objects; and both variants take the same ids
            run(k, 8)
            torch.cuda.synchronize()
            taken[k] = hist[1:9].cpu()
        ms = {k: [] for k in kinds}
        for _ in range(args.rounds):                             # alternating
            for k in kinds:
                ms[k].append(timed(k))
    best = {k: min(v) for k, v in ms.items()}
    return {"leg": "step_cost", "B": B, "context": f"{T}..{T + n}", "steps_per_sample": n, "samples_each": args.rounds,
            "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "ms_per_step_min": {k: round(v, 4) for k, v in best.items()},
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()}, "stops_over_null": round(best["stops4x16"] / best["null"], 4),
            "same_ids_with_and_without_the_table": bool(torch.equal(taken["null"], taken["stops4x16"]))}


def leg_queue(args) -> dict:
    import torch
    from visualcla import inflight as I
    from visualcla.synthetic import make_inputs
    model = _model(args)
    B, T, N = args.slots, args.prompt, args.requests
    b = budgets_of(args.seed, N)
    p = _cut_points(b, args.seed)
    px, ids, _ = make_inputs(model.config, N, T)
    px, ids = px.to(model.device, torch.bfloat16), ids.to(model.device)
    reqs = [dict(input_ids=ids[i], pixel_values=px[i], max_new_tokens=b[i]) for i in range(N)]
    kw = dict(max_batch=B, steps_per_sync=args.steps_per_sync, do_sample=False, eos_token_id=None)

    def go(rs, **extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = model.generate_many(rs, **kw, **extra)
        torch.cuda.synchronize()
        s = dict(model.last_inflight_stats)
        return [x.tolist() for x in o], time.perf_counter() - t0, s
    noop = lambda i, toks, fin: None                             # noqa: E731
    short = [dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])]
    go(short)                                                    # warm-up: every route once (code objects, both graphs)
    go([dict(r, stop_sequences=[[5, 6]]) for r in short], on_tokens=noop)
    free, t_free, s_free = go(reqs)
    assert [len(x) for x in free] == b
    stops = [[free[i][q - 2:q]] for i, q in enumerate(p)]
    want = [I.cut_at_stop(f, s) for f, s in zip(free, stops)]   # (a pair may occur before the point it was drawn from)
    got, t_stop, s_stop = go([dict(r, stop_sequences=s) for r, s in zip(reqs, stops)])
    sim, _ = I.simulate([len(w) for w in want], B, args.steps_per_sync)                # every stop hits where it was drawn
    sim_got, _ = I.simulate([len(g) for g in got], B, args.steps_per_sync)             # the lengths that came out
    _, t_stream, s_stream = go(reqs, on_tokens=noop)
    _, t_free2, _ = go(reqs)
    occ = lambda s: round(s["slot_steps_active"] / max(s["slot_steps_total"], 1), 4)      # noqa: E731
    boundaries = s_stream["steps"] // args.steps_per_sync
    return {"leg": "queue", "requests": N, "slots": B, "prompt": T, "budgeted_tokens": sum(b),
            "free": {"s": round(t_free, 3), "s_again": round(t_free2, 3), "steps": s_free["steps"], "occupancy": occ(s_free), "tokens": s_free["tokens"]},
            "stopped": {"s": round(t_stop, 3), "steps": s_stop["steps"], "occupancy": occ(s_stop), "tokens": s_stop["tokens"], "stop_hits": s_stop["stop_hits"],
                        "steps_the_host_simulation_predicts": sim.stats["steps"], "steps_it_predicts_for_the_lengths_that_came_out": sim_got.stats["steps"],
                        "requests_equal_to_the_cut_free_run": sum(g == w for g, w in zip(got, want)),
                        "requests_ending_on_a_stop": sum(I.stop_hit(g, s) for g, s in zip(got, stops))},
            "stopped_over_free": {"s": round(t_stop / t_free, 4), "steps": round(s_stop["steps"] / s_free["steps"], 4)},
            "streaming": {"s": round(t_stream, 3), "stream_calls": s_stream["stream_calls"], "boundaries": boundaries,
                          "added_ms_per_boundary": round((t_stream - min(t_free, t_free2)) * 1e3 / max(boundaries, 1), 4)},
            "note": "bf16 on random weights: stopping a request changes who is admitted together behind it, a prefill of another group size runs other GEMM "
                    "tiles, and a request whose rows round differently leaves its free run before the point its stop was drawn from -- it then runs to "
                    "its budget.  `requests_equal_to_the_cut_free_run` counts them; the fp32 tests assert equality"}


def _parent_step(args) -> dict:
    """the parent commit's own step_cost leg (its tools/inflight_probe.py, its library), as a child process from its tree"""
    cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.join("tools", "inflight_probe.py"), "--leg", "step_cost"] + \
          [x for k in ("slots", "prompt", "steps", "rounds", "layers") for x in (f"--{k}", str(getattr(args, k)))]
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "VCLA_LIB")}
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=args.parent_tree, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return {"leg": "parent_step_cost", "failed": r.returncode}
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return {"leg": "parent_step_cost", "tree": os.path.basename(os.path.abspath(args.parent_tree)), "slots_ms_per_step": d["ms_per_step"]["slots"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps-per-sync", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100, help="step_cost: steps per timed sample")
    ap.add_argument("--rounds", type=int, default=3, help="step_cost: alternating takes per variant")
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--leg", choices=["step_cost", "queue"], help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: its slots step is timed before and after ours")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "stop_sequences.txt"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps({"step_cost": leg_step_cost, "queue": leg_queue}[args.leg](args)), flush=True)
        return 0
    lines = [json.dumps(prediction(args))]
    print(lines[0], flush=True)
    if args.predict_only:
        return 0
    parent_ms, ours = [], None
    for leg in (["parent"] if args.parent_tree else []) + ["step_cost"] + (["parent"] if args.parent_tree else []) + ["queue"]:
        if leg == "parent":
            d = _parent_step(args)
            if "failed" in d:                                    # nothing more is started on the GPU after a failed leg
                print(f"stops_probe: the parent's step_cost leg failed with status {d['failed']}; stopping", file=sys.stderr)
                return d["failed"] or 1
            parent_ms += d["slots_ms_per_step"]
            line = json.dumps(d)
        else:
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg] + \
                  [x for k in ("requests", "slots", "prompt", "steps_per_sync", "seed", "steps", "rounds", "layers") for x in (f"--{k.replace('_', '-')}", str(getattr(args, k)))]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                # nothing more is started on the GPU after a failed leg
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                print(f"stops_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
                return r.returncode or 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            if leg == "step_cost":
                ours = json.loads(line)
        print(line, flush=True)
        lines.append(line)
        if leg == "parent" and ours is not None:                 # both sides of ours are in: the two conditions
            lo, hi = min(parent_ms), max(parent_ms)
            best = ours["ms_per_step_min"]
            line = json.dumps({"leg": "conditions", "parent_slots_ms_per_step": [round(x, 4) for x in parent_ms], "parent_min": round(lo, 4), "parent_spread_ms": round(hi - lo, 4),
                               "stops_over_parent": round(best["stops4x16"] / lo, 4), "stops_at_most_1.05x_parent": bool(best["stops4x16"] <= 1.05 * lo),
                               "null_minus_parent_ms": round(best["null"] - lo, 4), "null_within_parent_spread": bool(abs(best["null"] - lo) <= hi - lo)})
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/stops_probe.py on MI355X: one JSON line per leg (prediction: host arithmetic; the others: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

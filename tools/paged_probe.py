"""The paged K/V cache of the slots at the full 7B shape (synthetic weights as bench.py builds them, bf16): what the pool saves, what the
block table costs a slots step and an attention launch, and whether a queue that cannot be allocated contiguously runs.

    python tools/paged_probe.py [--requests 256] [--slots 64] [--prompt 128] [--steps-per-sync 8] [--seed 0] [--parent-tree DIR]
                                [--out profiles/paged_kv.txt]

The parent process never touches the GPU: it prints the accounting (host arithmetic, visualcla/inflight.py), then runs every GPU leg as
a child process under a time limit of its own and stops at the first leg that fails.  Every leg prints one JSON line; the parent writes
them to --out.

    step_cost   ms per graph-replayed slots step at B = slots, all slots active, argmax path: the contiguous cache (the launches of the commit
                before the pool) against the pool behind a block table whose blocks are scattered; `--rounds` takes of `--steps` steps each,
                alternating in one process.  --parent-tree DIR (a built checkout of the parent commit): its own tools/inflight_probe.py
                step_cost leg runs before and after ours, in the same session, and its `slots` step is the parent's figure; the same script
                runs over this tree's library too (the contiguous step measured exactly as the parent's).  Conditions: the paged step at most
                1.05 x the parent's; the contiguous step within the parent's spread
    attention   us per launch of vcla_attn_decode_paged against vcla_attn_decode_rows at B = slots, contexts 192 / 640 / 1900 (a report)
    queue       the inflight_probe queue (eos off) without a pool and with a pool of half the contiguous rows: wall time, kv_bytes against
                kv_bytes_contiguous, equal results (a report)
    long_queue  the same queue plus ONE request with a budget of 1900 at max_batch = --long-slots (256): contiguously B x 2048 rows, 256 GiB
                at 256 slots; with a pool of --long-pool-tokens rows.  Records whether it runs, and at what throughput (a report)
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

R = 16
ROW_7B = 2 * 32 * 4096 * 2      # bytes of one K/V row at the 7B shape in bf16


def accounting(args) -> dict:
    from visualcla import inflight as I
    b = budgets_of(args.seed, args.requests)
    out = {"leg": "accounting", "requests": args.requests, "prompt": args.prompt, "steps_per_sync": args.steps_per_sync, "budgeted_tokens": sum(b),
           "row_bytes": ROW_7B, "note": "host simulation with a pool as large as the contiguous cache: nothing waits, the peak is what the queue needs"}
    gib = lambda x: round(x / (1 << 30), 2)                      # noqa: E731
    for name, budgets in (("queue", b), ("queue_plus_one_1900", [1900] + b)):
        for slots in (64, 256):
            ref, _ = I.simulate(budgets, slots, args.steps_per_sync, prompt_lens=[args.prompt] * len(budgets), max_position_embeddings=2048)
            sch, _ = I.simulate(budgets, slots, args.steps_per_sync, prompt_lens=[args.prompt] * len(budgets), max_position_embeddings=2048,
                                kv_pool_tokens=slots * ref.ctx_max)
            acc = I.kv_accounting(sch, ROW_7B)
            out[f"{name}_{slots}_slots"] = {"ctx_max": sch.ctx_max, "contiguous_gib": gib(acc["kv_bytes_contiguous"]), "paged_peak_gib": gib(acc["kv_bytes_peak"]),
                                            "blocks_peak": sch.stats["kv_blocks_peak"], "rows_reserved_peak": sch.stats["kv_rows_reserved_peak"],
                                            "steps": sch.stats["steps"], "same_steps_as_without_a_pool": sch.stats["steps"] == ref.stats["steps"]}
    return out


def _scattered(rng, n_blocks, per_slot, B):
    free = list(range(n_blocks))
    rng.shuffle(free)
    return [[free.pop() for _ in range(per_slot)] for _ in range(B)]


def leg_step_cost(args) -> dict:
    import torch
    from visualcla import _lib
    model = _model(args)
    lib = _lib.load()
    dev = model.device
    t = model.config.text_config
    B, T, n, V = args.slots, args.prompt, args.steps, t["vocab_size"]
    ctx_max = (T + n + 2 + 63) // 64 * 64
    nL, H, d = t["num_hidden_layers"], t["num_attention_heads"], t["hidden_size"] // t["num_attention_heads"]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        kv = (torch.randn(nL, 2, B, H, ctx_max, d, device=dev) * 0.3).to(torch.bfloat16)
        per_slot = ctx_max // R
        NB = B * per_slot + 64
        blocks = _scattered(random.Random(args.seed), NB, per_slot, B)
        table = _lib.kv_page_rows(blocks, [ctx_max] * B, NB, per_slot).to(dev)
        pool = torch.zeros(nL, 2, H, NB * R, d, dtype=torch.bfloat16, device=dev)
        for b in range(B):                                       # the same rows behind the table
            idx = torch.tensor([blocks[b][r // R] * R + r % R for r in range(ctx_max)], device=dev)
            pool[:, :, :, idx] = kv[:, :, b]
        pages = _lib.kv_pages(table, NB)
        km = torch.ones(B, ctx_max, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.vcla_llama_workspace_bytes(model._ctx, B, 1) + 512, dtype=torch.uint8, device=dev)
        ids = torch.randint(3, V - 8, (B,), generator=torch.Generator().manual_seed(3)).to(dev)
        W = _lib.SLOT_SUMMARY_WORDS
        st = torch.zeros(4 * B + W, dtype=torch.int32, device=dev)
        hist = torch.zeros(n + 2, B, dtype=torch.int64, device=dev)
        cur = ids.clone()
        slots = _lib.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
        init = torch.tensor([T] * B + [1] * B + [1] * B + [n + 2] * B + [0] * W, dtype=torch.int32, device=dev)

        def run(kind, steps):
            st.copy_(init)
            cur.copy_(ids)
            args_ = (model._ctx, C.byref(slots), steps, (pool if kind == "paged" else kv).data_ptr(), ctx_max, km.data_ptr(), ws.data_ptr(), ws.numel(), 1,
                     None, None, None, None, None, None)
            if kind == "paged":
                _lib.check(lib.vcla_llama_decode_slots_paged(*args_, C.byref(pages), _lib.stream_ptr()))
            else:
                _lib.check(lib.vcla_llama_decode_slots_stops(*args_, _lib.stream_ptr()))

        def timed(kind):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run(kind, 1)                                         # one graph slot, alternating keys: the capture happens here, untimed
            e0.record(stream)
            run(kind, n)
            e1.record(stream)
            torch.cuda.synchronize()
            assert st[4 * B].item() == B and st[:B].tolist() == [T + n] * B, "every slot must still be active"
            return e0.elapsed_time(e1) / n
        kinds = ("contiguous", "paged")
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
    return {"leg": "step_cost", "B": B, "context": f"{T}..{T + n}", "steps_per_sample": n, "samples_each": args.rounds, "pool_blocks": NB,
            "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "ms_per_step_min": {k: round(v, 4) for k, v in best.items()},
            "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()}, "paged_over_contiguous": round(best["paged"] / best["contiguous"], 4),
            "same_ids_with_and_without_the_table": bool(torch.equal(taken["contiguous"], taken["paged"]))}


def leg_attention(args) -> dict:
    import torch
    from visualcla import _lib
    _lib.require_device()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, H, d, reps = args.slots, 32, 128, 200
    out = {"leg": "attention", "B": B, "H": H, "d": d, "launches_per_sample": reps, "us_per_launch": {}}
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for ctx in (192, 640, 1900):
            cap = (ctx + 2 + 63) // 64 * 64
            g = torch.Generator(device=dev).manual_seed(ctx)
            ang = torch.rand(cap, d // 2, generator=g, device=dev) * 6.28
            cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
            kv = (torch.randn(2, B, H, cap, d, generator=g, device=dev) * 0.5).to(torch.bfloat16)
            qkv = torch.randn(B, 3 * H * d, generator=g, device=dev).to(torch.bfloat16)
            km = torch.ones(B, cap, dtype=torch.int32, device=dev)
            o = torch.zeros((H * d) // 32, (B + 15) // 16, 64, 8, dtype=torch.bfloat16, device=dev)
            row_pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
            per_slot = cap // R
            NB = B * per_slot + 64
            blocks = _scattered(random.Random(ctx), NB, per_slot, B)
            table = _lib.kv_page_rows(blocks, [cap] * B, NB, per_slot).to(dev)
            pool = torch.zeros(2, H, NB * R, d, dtype=torch.bfloat16, device=dev)
            for b in range(B):
                idx = torch.tensor([blocks[b][r // R] * R + r % R for r in range(cap)], device=dev)
                pool[:, :, idx] = kv[:, b]
            pages = _lib.kv_pages(table, NB)
            scale = d ** -0.5

            def rows():
                _lib.check(lib.vcla_attn_decode_rows(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), o.data_ptr(), B, H, d, cap,
                                                     row_pos.data_ptr(), km.data_ptr(), cap, scale, _lib.VCLA_BF16, 1, _lib.stream_ptr()))

            def paged():
                _lib.check(lib.vcla_attn_decode_paged(qkv.data_ptr(), pool[0].data_ptr(), pool[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), o.data_ptr(), B, H, d, cap,
                                                      row_pos.data_ptr(), C.byref(pages), km.data_ptr(), cap, scale, _lib.VCLA_BF16, 1, _lib.stream_ptr()))
            res = {"rows": [], "paged": []}
            for fn in (rows, paged):
                for _ in range(10):
                    fn()
            for _ in range(args.rounds):
                for name, fn in (("rows", rows), ("paged", paged)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(reps):
                        fn()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    res[name].append(round(e0.elapsed_time(e1) * 1e3 / reps, 2))
            out["us_per_launch"][str(ctx)] = dict(res, paged_over_rows=round(min(res["paged"]) / min(res["rows"]), 4))
            del kv, pool
    out["note"] = "back-to-back launches on one stream, every slot at the stated context, the same rows behind a scattered table"
    return out


def _queue_requests(args, model, budgets):
    import torch
    from visualcla.synthetic import make_inputs
    N = len(budgets)
    px, ids, _ = make_inputs(model.config, N, args.prompt)
    px, ids = px.to(model.device, torch.bfloat16), ids.to(model.device)
    return [dict(input_ids=ids[i], pixel_values=px[i], max_new_tokens=budgets[i]) for i in range(N)]


def _go(model, rs, **kw):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = model.generate_many(rs, **kw)
    torch.cuda.synchronize()
    return [x.tolist() for x in o], time.perf_counter() - t0, dict(model.last_inflight_stats)


def leg_queue(args) -> dict:
    model = _model(args)
    B = args.slots
    b = budgets_of(args.seed, args.requests)
    reqs = _queue_requests(args, model, b)
    kw = dict(max_batch=B, steps_per_sync=args.steps_per_sync, do_sample=False, eos_token_id=None)
    short = [dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])]
    _go(model, short, **kw)                                      # warm-up: both routes once (code objects, both graphs)
    _go(model, short, kv_pool_tokens=B * 256, **kw)
    free, t_free, s_free = _go(model, reqs, **kw)
    pool_tokens = B * s_free["ctx_max"] // 2
    got, t_pool, s_pool = _go(model, reqs, kv_pool_tokens=pool_tokens, **kw)
    _, t_free2, _ = _go(model, reqs, **kw)
    keys = ("kv_pool_blocks", "kv_blocks_peak", "kv_bytes", "kv_bytes_contiguous", "kv_rows_reserved_peak", "admission_waits_blocks", "steps", "admission_groups")
    return {"leg": "queue", "requests": len(reqs), "slots": B, "prompt": args.prompt, "budgeted_tokens": sum(b),
            "without_a_pool": {"s": round(t_free, 3), "s_again": round(t_free2, 3), "steps": s_free["steps"], "ctx_max": s_free["ctx_max"],
                               "tok_per_s": round(sum(b) / min(t_free, t_free2), 1)},
            "with_a_pool": dict({k: s_pool[k] for k in keys}, s=round(t_pool, 3), kv_pool_tokens=pool_tokens, tok_per_s=round(sum(b) / t_pool, 1)),
            "pool_over_none_s": round(t_pool / min(t_free, t_free2), 4), "requests_with_equal_results": sum(x == y for x, y in zip(free, got))}


def leg_long_queue(args) -> dict:
    model = _model(args)
    B = args.long_slots
    b = [1900] + budgets_of(args.seed, args.requests)
    reqs = _queue_requests(args, model, b)
    kw = dict(max_batch=B, steps_per_sync=args.steps_per_sync, do_sample=False, eos_token_id=None)
    _go(model, [dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])], kv_pool_tokens=B * 256, **kw)      # warm-up
    got, t_pool, s = _go(model, reqs, kv_pool_tokens=args.long_pool_tokens, **kw)
    keys = ("kv_pool_blocks", "kv_blocks_peak", "kv_bytes", "kv_bytes_contiguous", "kv_rows_reserved_peak", "admission_waits_blocks", "steps", "ctx_max", "slots")
    return {"leg": "long_queue", "requests": len(reqs), "max_batch": B, "budgeted_tokens": sum(b), "ran": [len(x) for x in got] == b,
            "s": round(t_pool, 3), "tok_per_s": round(sum(b) / t_pool, 1), "kv_pool_tokens": args.long_pool_tokens, **{k: s[k] for k in keys},
            "kv_gib": round(s["kv_bytes"] / (1 << 30), 2), "kv_contiguous_gib": round(s["kv_bytes_contiguous"] / (1 << 30), 2)}


def _parent_step(args, tree=None) -> dict:
    """the step_cost leg of tools/inflight_probe.py as a child process: from the parent commit's tree (its script, its library), or with
    tree=ROOT the SAME script over this tree's library -- the contiguous step measured exactly as the parent's is"""
    name = "parent_step_cost" if tree is None else "own_step_cost"
    tree = args.parent_tree if tree is None else tree
    cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.join("tools", "inflight_probe.py"), "--leg", "step_cost"] + \
          [x for k in ("slots", "prompt", "steps", "rounds", "layers") for x in (f"--{k}", str(getattr(args, k)))]
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "VCLA_LIB")}
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return {"leg": name, "failed": r.returncode}
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return {"leg": name, "tree": os.path.basename(os.path.abspath(tree)), "slots_ms_per_step": d["ms_per_step"]["slots"]}


LEGS = {"step_cost": leg_step_cost, "attention": leg_attention, "queue": leg_queue, "long_queue": leg_long_queue}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps-per-sync", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100, help="step_cost: steps per timed sample")
    ap.add_argument("--rounds", type=int, default=3, help="step_cost / attention: alternating takes per variant")
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--long-slots", type=int, default=256, help="long_queue: max_batch")
    ap.add_argument("--long-pool-tokens", type=int, default=80 * 1024, help="long_queue: rows of the pool (80 Ki rows = 40 GiB at the 7B shape)")
    ap.add_argument("--leg", choices=sorted(LEGS), help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--legs", default="step_cost,attention,queue,long_queue", help="the GPU legs to run, in this order")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: its slots step is timed before and after ours")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "paged_kv.txt"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(LEGS[args.leg](args)), flush=True)
        return 0
    lines = [json.dumps(accounting(args))]
    print(lines[0], flush=True)
    if args.predict_only:
        return 0
    parent_ms, own_ms, ours = [], [], None
    order = []
    for leg in [x for x in args.legs.split(",") if x]:
        order += (["parent", "own", leg, "own", "parent"] if leg == "step_cost" and args.parent_tree else [leg])
    for leg in order:
        if leg in ("parent", "own"):
            d = _parent_step(args, None if leg == "parent" else ROOT)
            if "failed" in d:                                    # nothing more is started on the GPU after a failed leg
                print(f"paged_probe: the {leg} step_cost leg of tools/inflight_probe.py failed with status {d['failed']}; stopping", file=sys.stderr)
                return d["failed"] or 1
            (parent_ms if leg == "parent" else own_ms).extend(d["slots_ms_per_step"])
            line = json.dumps(d)
        else:
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg] + \
                  [x for k in ("requests", "slots", "prompt", "steps_per_sync", "seed", "steps", "rounds", "layers", "long_slots", "long_pool_tokens")
                   for x in (f"--{k.replace('_', '-')}", str(getattr(args, k)))]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                                # nothing more is started on the GPU after a failed leg
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                print(f"paged_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
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
                               "paged_over_parent": round(best["paged"] / lo, 4), "paged_at_most_1.05x_parent": bool(best["paged"] <= 1.05 * lo),
                               "contiguous_ms_per_step_same_script": [round(x, 4) for x in own_ms], "contiguous_minus_parent_ms": round(min(own_ms) - lo, 4),
                               "contiguous_within_parent_spread": bool(abs(min(own_ms) - lo) <= hi - lo),
                               "contiguous_in_the_paged_leg_minus_parent_ms": round(best["contiguous"] - lo, 4),
                               "note": "contiguous: this tree's library under the parent's own measuring script (tools/inflight_probe.py), so that "
                                       "only the library differs; the step_cost leg's contiguous figure shares its process with the pool"})
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/paged_probe.py on MI355X: one JSON line per leg (accounting: host arithmetic; the others: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

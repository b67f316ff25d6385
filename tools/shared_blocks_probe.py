"""Prompt blocks shared by reference in the paged K/V pool at the full 7B shape (synthetic weights as bench.py builds them, bf16): what the
paged form of the ragged admission pass costs, what sharing by reference buys one boundary, what it costs a queue that shares nothing, and
what the 16 x 16 queue holds at its peak.

    python tools/shared_blocks_probe.py [--requests 256] [--slots 64] [--images 16] [--steps-per-sync 8] [--seed 0] [--parent-tree DIR]
                                        [--out profiles/shared_blocks.txt]

The parent process never touches the GPU: it prints the accounting (host arithmetic: visualcla/prefix.py at block granularity, the scheduler of
visualcla/inflight.py under its fake stepper), then runs every GPU leg as a child process under a time limit of its own and stops at the
first leg that fails.  Every leg prints one JSON line; the parent writes them to --out.

    pass        ms per vcla_llama_extend_rows_paged against vcla_llama_extend_rows on the nine tables of tools/prefix_probe.py's kernel leg
                (4 / 16 / 64 sequences x R38_p90 / R128_p0 / mixed), the same rows behind a scattered table, alternating takes in one process;
                the attention launch alone beside it (a report).  --parent-tree DIR (a built checkout of the parent commit): the contiguous
                side runs in a child over the PARENT's library (VCLA_LIB) before and after ours, and the condition -- at most 1.05 x on
                each table -- is taken against it
    boundary    one boundary of 64 requests about 4 images at budget 1 with a pool: share_blocks=True against the padded admission (the
                parent's only option with a pool); share_prefix=True without a pool beside it (a report)
    distinct    a queue of 256 distinct images with a pool, share_blocks=True against the call without it (condition: at most 1.05 x)
    queue       the 16 x 16 queue with share_blocks at --slots and at 256 slots: time, peak blocks against the accounting, waits (a report)
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
from prefix_probe import bench_prompts  # noqa: E402

R = 16
ROW_7B = 2 * 32 * 4096 * 2      # bytes of one K/V row at the 7B shape in bf16
CTX = 2048
MIXED_R, MIXED_P = [38, 128, 5, 64, 100, 17, 256, 38], [90, 0, 700, 25, 0, 1900, 0, 90]


def tables():
    for n in (4, 16, 64):
        yield n, "R38_p90", [(b, 90, 38) for b in range(n)]
        yield n, "R128_p0", [(b, 0, 128) for b in range(n)]
        yield n, "mixed", [(b, min(MIXED_P[b % 8], CTX - MIXED_R[b % 8]), MIXED_R[b % 8]) for b in range(n)]


def accounting(args) -> dict:
    from visualcla import inflight as I
    from visualcla import prefix
    prompts, image_of, tok = bench_prompts(args.images, args.requests // args.images, False, args.seed)
    b = budgets_of(args.seed, len(prompts))
    T = [len(p) for p in prompts]
    exact = prefix.plan(prompts, image_of, tok, args.slots)
    out = {"leg": "accounting", "requests": len(prompts), "images": args.images, "rows_without": sum(T), "rows_computed_exact_plan": exact.rows_computed,
           "row_bytes": ROW_7B, "note": "host simulation with an ample pool: nothing waits, the peak is what the queue holds"}
    for slots in (64, 256):
        pl = prefix.plan(prompts, image_of, tok, slots, block_rows=R)
        kw = dict(prompt_lens=T, has_image=[True] * len(T), max_position_embeddings=2048)
        plain, _ = I.simulate(b, slots, args.steps_per_sync, kv_pool_tokens=slots * 640, **kw)
        sch, _ = I.simulate(b, slots, args.steps_per_sync, kv_pool_tokens=slots * 640, block_plan=pl, **kw)
        out[f"{slots}_slots"] = {"rows_computed": pl.rows_computed, "vision_runs": pl.vision_runs, "blocks_peak_without": plain.stats["kv_blocks_peak"],
                                 "blocks_peak_with": sch.stats["kv_blocks_peak"], "gib_peak_without": round(plain.stats["kv_blocks_peak"] * R * ROW_7B / (1 << 30), 2),
                                 "gib_peak_with": round(sch.stats["kv_blocks_peak"] * R * ROW_7B / (1 << 30), 2), "blocks_shared_peak": sch.stats["kv_blocks_shared_peak"],
                                 "rows_by_reference": sch.stats["kv_rows_shared"], "entry_bound_blocks": sch.entry_bound, "steps": sch.stats["steps"]}
    return out


def _paged_copy(torch, _lib, rng, kv, table, dev):
    """kv [L, 2, n, H, CTX, d] -> (pool [L, 2, H, NB * 16, d] holding the same rows behind a scattered table, Pages-like object)"""
    n = kv.shape[2]
    need = {s: (p + r + R - 1) // R for s, p, r in table}
    NB = sum(need.values()) + 64
    free = list(range(NB))
    rng.shuffle(free)
    blocks = [[free.pop() for _ in range(need[s])] for s in range(n)]
    tab = _lib.kv_page_rows(blocks, [p + r for _, p, r in sorted(table)], NB, CTX // R).to(dev)
    pool = torch.zeros(kv.shape[0], 2, kv.shape[3], NB * R, kv.shape[5], dtype=kv.dtype, device=dev)
    for s in range(n):
        idx = torch.tensor([blocks[s][r // R] * R + r % R for r in range(need[s] * R)], device=dev)
        pool[:, :, :, idx] = kv[:, :, s, :, :need[s] * R]

    class Pg:
        pass
    pg = Pg()
    pg.table, pg.args = tab, _lib.kv_pages(tab, NB)
    return pool, pg


def leg_pass(args) -> dict:
    import torch
    from visualcla import _lib
    from visualcla.weights import rope_tables
    if args.contiguous_only:                                     # the parent's library lacks the new entries: do not ask it for them
        for name in ("vcla_attn_extend_rows_paged", "vcla_llama_extend_rows_paged"):
            _lib.SYMBOLS.pop(name, None)
    model = _model(args)
    lib = _lib.load()
    dev = model.device
    t = model.config.text_config
    nL, H, d, D = t["num_hidden_layers"], t["num_attention_heads"], t["hidden_size"] // t["num_attention_heads"], t["hidden_size"]
    paged_lib = not args.contiguous_only
    stream = torch.cuda.Stream(device=dev)
    rows = []
    g = torch.Generator().manual_seed(0)
    cos, sin = (x.to(dev) for x in rope_tables(CTX, d, 10000.0))
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for n, name, table in tables():
            kv = torch.empty(nL, 2, n, H, CTX, d, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.3)
            M = sum(r for _, _, r in table)
            emb = (torch.randn(M, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            forms = {"contiguous": lambda: model._extend_rows(emb, table, kv)}
            if paged_lib:
                pool, pg = _paged_copy(torch, _lib, random.Random(n), kv, table, dev)
                forms["paged"] = lambda: model._extend_rows(emb, table, pool, pages=pg, ctx_max=CTX)
                seqs, _ = _lib.extend_seqs(table)
                qkv = torch.randn(M, 3 * H * d, generator=g).to(torch.bfloat16).to(dev)
                o = torch.zeros(M, H * d, dtype=torch.bfloat16, device=dev)
                sc = torch.empty(lib.vcla_attn_extend_rows_scratch_bytes(seqs, n, H, d), dtype=torch.uint8, device=dev)
                head = (qkv.data_ptr(), None, None, cos.data_ptr(), sin.data_ptr(), o.data_ptr(), seqs, n, M, n, H, d, CTX, d ** -0.5, _lib.VCLA_BF16, 0, 0,
                        sc.data_ptr(), sc.numel())
                attn = {"attn_contiguous": lambda: _lib.check(lib.vcla_attn_extend_rows(head[0], kv[0, 0].data_ptr(), kv[0, 1].data_ptr(), *head[3:], _lib.stream_ptr())),
                        "attn_paged": lambda: _lib.check(lib.vcla_attn_extend_rows_paged(head[0], pool[0, 0].data_ptr(), pool[0, 1].data_ptr(), *head[3:],
                                                                                         C.byref(pg.args), _lib.stream_ptr()))}
            ms = {k: [] for k in forms}
            for fn in forms.values():
                fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):                         # alternating takes
                for k, fn in forms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.reps):
                        fn()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    ms[k].append(round(e0.elapsed_time(e1) / args.reps, 4))
            row = {"n": n, "table": name, "M": M, "ms": ms}
            if paged_lib:
                us = {k: [] for k in attn}
                for _ in range(args.rounds):
                    for k, fn in attn.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(50):
                            fn()
                        e1.record(stream)
                        torch.cuda.synchronize()
                        us[k].append(round(e0.elapsed_time(e1) * 1000 / 50, 2))
                row.update(paged_over_contiguous=round(min(ms["paged"]) / min(ms["contiguous"]), 4), attention_us={k: min(v) for k, v in us.items()},
                           attention_paged_over_contiguous=round(min(us["attn_paged"]) / min(us["attn_contiguous"]), 4))
                del pool
            rows.append(row)
            del kv
    return {"leg": "pass", "library": os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(_lib.LIB_PATH)))), "layers": nL, "reps": args.reps,
            "rounds": args.rounds, "tables": rows}


def _boundary_requests(args, model, n_img, B):
    import torch
    from visualcla.synthetic import make_inputs
    prompts, image_of, _ = bench_prompts(n_img, B // n_img, False, args.seed)
    px, _, _ = make_inputs(model.config, n_img, 128)
    px = px.to(model.device, torch.bfloat16)
    ids = torch.tensor(prompts, device=model.device)
    return [dict(input_ids=ids[i], pixel_values=px[image_of[i]].clone(), max_new_tokens=1) for i in range(len(prompts))]


def _ms(model, reqs, **kw):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate_many(reqs, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000, out


def leg_boundary(args) -> dict:
    model = _model(args)
    B = args.slots
    reqs = _boundary_requests(args, model, 4, B)
    kw = dict(do_sample=False, eos_token_id=None, max_batch=B)
    pool = B * 256
    forms = {"paged_padded": dict(kv_pool_tokens=pool), "share_blocks": dict(kv_pool_tokens=pool, share_blocks=True), "share_prefix_no_pool": dict(share_prefix=True)}
    for _ in range(2):
        for f in forms.values():
            _ms(model, reqs, **kw, **f)
    takes = []
    for _ in range(2):
        ms = {k: [] for k in forms}
        for _ in range(3):
            for k, f in forms.items():
                ms[k].append(_ms(model, reqs, **kw, **f)[0])
        takes.append({k: round(min(v), 3) for k, v in ms.items()})
    _ms(model, reqs, **kw, **forms["share_blocks"])
    st = dict(model.last_inflight_stats)
    best = {k: min(t[k] for t in takes) for k in forms}
    return {"leg": "boundary", "requests": B, "images": 4, "ms_take1": takes[0], "ms_take2": takes[1], "share_blocks_over_paged_padded": round(best["share_blocks"] / best["paged_padded"], 4),
            "share_blocks_faster_than_paged_padded": bool(best["share_blocks"] < best["paged_padded"]),
            **{k: st[k] for k in ("rows_reused", "rows_computed", "vision_runs", "admission_passes", "kv_rows_shared", "kv_blocks_peak", "kv_blocks_shared_peak")}}


def _queue_run(args, model, reqs, b, B, **extra):
    kw = dict(do_sample=False, eos_token_id=None, max_batch=B, steps_per_sync=args.steps_per_sync)
    ms, got = _ms(model, reqs, **kw, **extra)
    assert [len(x) for x in got] == b
    st = model.last_inflight_stats
    return {"s": round(ms / 1000, 3), "admission_s": round(st["admission_s"], 3), "steps": st["steps"],
            **{k: st[k] for k in ("kv_blocks_peak", "kv_blocks_shared_peak", "kv_rows_shared", "admission_waits_blocks", "rows_computed", "vision_runs") if k in st}}


def leg_distinct(args) -> dict:
    from prefix_probe import _queue
    model = _model(args)
    B, N = args.slots, args.requests
    b = budgets_of(args.seed, N)
    reqs = _queue(args, model, True, N, b)
    pool = B * 640
    warm = [dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])]
    for extra in (dict(kv_pool_tokens=pool), dict(kv_pool_tokens=pool, share_blocks=True)):
        model.generate_many(warm, do_sample=False, eos_token_id=None, max_batch=B, steps_per_sync=args.steps_per_sync, **extra)
    takes = []
    for _ in range(2):
        takes.append({"paged": _queue_run(args, model, reqs, b, B, kv_pool_tokens=pool), "share_blocks": _queue_run(args, model, reqs, b, B, kv_pool_tokens=pool, share_blocks=True)})
    best = {k: min(t[k]["s"] for t in takes) for k in ("paged", "share_blocks")}
    return {"leg": "distinct", "requests": N, "slots": B, "takes": takes, "best_s": best, "share_blocks_over_paged": round(best["share_blocks"] / best["paged"], 4),
            "at_most_1.05x": bool(best["share_blocks"] <= 1.05 * best["paged"])}


def leg_queue(args) -> dict:
    from prefix_probe import _queue
    model = _model(args)
    N = args.requests
    b = budgets_of(args.seed, N)
    reqs = _queue(args, model, False, N, b)
    out = {"leg": "queue", "requests": N, "images": args.images}
    for B in (args.slots, 256):
        pool = B * 640
        model.generate_many([dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:min(N, B + 8)])], do_sample=False, eos_token_id=None, max_batch=B,
                            steps_per_sync=args.steps_per_sync, kv_pool_tokens=pool, share_blocks=True)
        out[f"{B}_slots"] = {"share_blocks": _queue_run(args, model, reqs, b, B, kv_pool_tokens=pool, share_blocks=True), "paged": _queue_run(args, model, reqs, b, B, kv_pool_tokens=pool)}
    return out


LEGS = {"pass": leg_pass, "boundary": leg_boundary, "distinct": leg_distinct, "queue": leg_queue}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps-per-sync", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5, help="pass: calls per timed sample")
    ap.add_argument("--rounds", type=int, default=3, help="pass: alternating takes per form")
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--contiguous-only", action="store_true", help="pass: time vcla_llama_extend_rows alone (what the parent spawns over the parent's library)")
    ap.add_argument("--leg", choices=sorted(LEGS), help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--legs", default="pass,boundary,distinct,queue", help="the GPU legs to run, in this order")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: its library runs the contiguous pass before and after ours")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "shared_blocks.txt"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(LEGS[args.leg](args)), flush=True)
        return 0
    lines = [json.dumps(accounting(args))]
    print(lines[0], flush=True)
    if args.predict_only:
        return 0
    common = [x for k in ("requests", "slots", "images", "prompt", "steps_per_sync", "seed", "reps", "rounds", "layers") for x in (f"--{k.replace('_', '-')}", str(getattr(args, k)))]
    order = []
    for leg in [x for x in args.legs.split(",") if x]:
        order += (["parent", leg, "parent"] if leg == "pass" and args.parent_tree else [leg])
    parent, ours = [], None
    for leg in order:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "pass" if leg == "parent" else leg] + common
        env = dict(os.environ)
        if leg == "parent":                                      # this script, the parent's library: only the library differs
            cmd.append("--contiguous-only")
            env["VCLA_LIB"] = os.path.join(os.path.abspath(args.parent_tree), "visual-chinese-llama-alpaca_amd", "visualcla", "libvisualcla_hip.so")
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        if r.returncode != 0:                                    # nothing more is started on the GPU after a failed leg
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"shared_blocks_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        d = json.loads(line)
        if leg == "parent":
            d["leg"] = "pass_parent_library"
            parent.append(d)
            line = json.dumps(d)
        elif leg == "pass":
            ours = d
        print(line, flush=True)
        lines.append(line)
        if leg == "parent" and ours is not None:
            cond = []
            for k, row in enumerate(ours["tables"]):
                base = min(x for p in parent for x in p["tables"][k]["ms"]["contiguous"])
                cond.append({"n": row["n"], "table": row["table"], "parent_ms": base, "paged_ms": min(row["ms"]["paged"]), "paged_over_parent": round(min(row["ms"]["paged"]) / base, 4)})
            line = json.dumps({"leg": "conditions", "tables": cond, "every_table_at_most_1.05x": all(c["paged_over_parent"] <= 1.05 for c in cond)})
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/shared_blocks_probe.py on MI355X: one JSON line per leg (accounting: host arithmetic; the others: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Prefix sharing at the full 7B shape (synthetic weights as bench.py builds them, bf16): what the ragged attention kernel costs next to the
launches that do the same work without it, what one admission boundary costs with and without sharing, and what generate_many(share_prefix=True)
buys on a queue that shares (16 images x 16 questions) and costs on one that does not (256 distinct images).

    python tools/prefix_probe.py [--requests 256] [--slots 64] [--images 16] [--steps-per-sync 8] [--seed 0] [--out profiles/prefix_sharing.txt]

The parent process never touches the GPU: it prints the row accounting (host arithmetic, visualcla/prefix.py), then runs every GPU leg as a
child process under a time limit of its own and stops at the first leg that fails.  Every leg prints one JSON line; the parent writes them
to --out.  Every table is taken twice in one process, the legs alternating, and the spread between the two takes is printed beside it.

    kernel      vcla_attn_extend_rows for 4 / 16 / 64 sequences at (R, p) = (38, 90), (128, 0) and a mixed table, us per layer, against
                vcla_attn_extend once per sequence and (p = 0, equal lengths) vcla_rope_kv_append + vcla_attention on the padded batch
    admission   one boundary of 64 requests (16 questions x 4 images, T = 128, slot ending at row 90): ms with share_prefix on against off,
                the `on` side split into vision / pool copies / rows pass (a synchronise between the parts, in a run of its own)
    queue_a     256 requests = 16 images x 16 questions, budgets of tools/inflight_probe.py: useful tok/s, admission_s, on against off
    queue_b     256 distinct images (nothing to share): the same, on against off
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

import numpy as np  # noqa: E402

from inflight_probe import _model, budgets_of  # noqa: E402

H, D, CTX = 32, 128, 2048


def bench_prompts(n_images: int, n_questions: int, common_head: bool, seed: int = 0):
    """ids laid out as bench.py lays its prompt out: BOS + 23 ids + <img> + 64 <img_token> + </img> + 38 ids = 128 rows; arrival interleaved by
    image.  -> (list of id lists, image index per request)"""
    from visualcla.synthetic import stub_tokenizer
    tk = stub_tokenizer()
    rng = np.random.default_rng(seed + 77)
    lo, hi = 3, min(tk.img_start_token_id, tk.img_end_token_id, tk.img_token_id)
    heads = [rng.integers(lo, hi, 23).tolist() for _ in range(n_images)]
    for k in range(n_images):
        heads[k][0] = lo + k                                     # distinct from the first id on
    if common_head:
        heads = [heads[0]] * n_images
    prompts, image_of = [], []
    for q in range(n_questions):
        for k in range(n_images):
            tail = rng.integers(lo, hi, 38).tolist()
            tail[0] = lo + (q * n_images + k) % (hi - lo)
            prompts.append([1] + heads[k] + [tk.img_start_token_id] + [tk.img_token_id] * 64 + [tk.img_end_token_id] + tail)
            image_of.append(k)
    return prompts, image_of, tk.img_token_id


def prediction(args) -> dict:
    from visualcla import prefix
    prompts, image_of, tok = bench_prompts(args.images, args.requests // args.images, False, args.seed)
    pl = prefix.plan(prompts, image_of, tok, args.slots)
    first = prefix.passes(pl, list(range(min(args.slots, len(prompts)))))
    return {"leg": "prediction", "requests": len(prompts), "images": args.images, "rows_without": sum(pl.T), "rows_computed": pl.rows_computed,
            "rows_reused": pl.rows_reused, "share_of_rows_computed": round(pl.rows_computed / sum(pl.T), 4), "vision_runs": pl.vision_runs,
            "pool_entries": len(pl.entries), "pool_rows": pl.peak_pool_rows, "passes_of_boundary_0": [len(p) for p in first]}


def _alternate(torch, stream, forms, takes=2, rounds=3, reps=20):
    """us per call of every form: `takes` tables, each the minimum over `rounds` alternating samples of `reps` calls"""
    tables = []
    for _ in range(takes):
        us = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1000 / reps)
        tables.append({k: round(min(v), 2) for k, v in us.items()})
    return tables


def leg_kernel(args) -> dict:
    import torch
    from visualcla import _lib
    from visualcla.weights import rope_tables
    _lib.require_device()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    cos, sin = (t.to(dev) for t in rope_tables(CTX, D, 10000.0))
    scale = D ** -0.5
    stream = torch.cuda.Stream(device=dev)
    rows = []
    mixed_r, mixed_p = [38, 128, 5, 64, 100, 17, 256, 38], [90, 0, 700, 25, 0, 1900, 0, 90]
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for n in (4, 16, 64):
            kv = (torch.randn(2, n, H, CTX, D, device=dev) * 0.5).to(torch.bfloat16)
            ctx = CTX
            for name, table in (("R38_p90", [(b, 90, 38) for b in range(n)]), ("R128_p0", [(b, 0, 128) for b in range(n)]),
                                ("mixed", [(b, min(mixed_p[b % 8], ctx - mixed_r[b % 8]), mixed_r[b % 8]) for b in range(n)])):
                seqs, M = _lib.extend_seqs(table)
                qkv0 = torch.randn(M, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
                qkv = qkv0.clone()
                out_r, out_x, out_p = (torch.zeros(M, H * D, dtype=torch.bfloat16, device=dev) for _ in range(3))
                sr = torch.empty(lib.vcla_attn_extend_rows_scratch_bytes(seqs, n, H, D), dtype=torch.uint8, device=dev)
                sx = torch.empty(max(max(lib.vcla_attn_extend_scratch_bytes(r, H, D, p) for _, p, r in table), 16), dtype=torch.uint8, device=dev)

                def ragged():
                    _lib.check(lib.vcla_attn_extend_rows(qkv0.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_r.data_ptr(), seqs, n,
                                                         M, n, H, D, ctx, scale, _lib.VCLA_BF16, 0, 0, sr.data_ptr(), sr.numel(), _lib.stream_ptr()))

                def per_sequence():
                    m0 = 0
                    for b, p, r in table:
                        _lib.check(lib.vcla_attn_extend(qkv0[m0:].data_ptr(), kv[0, b].data_ptr(), kv[1, b].data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                        out_x[m0:].data_ptr(), r, H, D, ctx, p, scale, _lib.VCLA_BF16, 0, sx.data_ptr(), sx.numel(), _lib.stream_ptr()))
                        m0 += r
                forms = {"ragged": ragged, "per_sequence": per_sequence}
                if name == "R128_p0":
                    T = 128
                    a = _lib.AttnArgs()
                    a.q, a.k, a.v, a.o = qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), out_p.data_ptr()
                    a.q_bs, a.q_hs, a.q_rs = T * 3 * H * D, D, 3 * H * D
                    a.k_bs = a.v_bs = H * ctx * D
                    a.k_hs = a.v_hs = ctx * D
                    a.k_rs = a.v_rs = D
                    a.o_bs, a.o_hs, a.o_rs = T * H * D, D, H * D
                    a.B, a.H, a.Tq, a.Tk, a.D, a.scale, a.causal = n, H, T, T, D, scale, 1

                    def pair():
                        _lib.check(lib.vcla_rope_kv_append(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), n, T, H, D, ctx, 0,
                                                           None, _lib.VCLA_BF16, _lib.stream_ptr()))
                        _lib.check(lib.vcla_attention(C.byref(a), _lib.VCLA_BF16, _lib.stream_ptr()))
                    forms["padded_pair"] = pair
                for fn in forms.values():                        # the outputs at this size, from one qkv (the pair rotates its copy in place: first call only)
                    fn()
                torch.cuda.synchronize()
                diff = {k: float((o.float() - out_r.float()).abs().max()) for k, o in (("per_sequence", out_x), ("padded_pair", out_p)) if k in forms}
                assert all(v <= 1.6e-2 for v in diff.values()), (n, name, diff)
                for fn in forms.values():
                    for _ in range(5):
                        fn()
                t1, t2 = _alternate(torch, stream, forms)
                rows.append({"n_seqs": n, "table": name, "M": M, "us_take1": t1, "us_take2": t2,
                             "spread": round(max(abs(t1[k] - t2[k]) / min(t1[k], t2[k]) for k in t1), 4),
                             "max_abs_diff_vs_ragged": {k: round(v, 5) for k, v in diff.items()}})
    return {"leg": "kernel", "H": H, "d": D, "calls_per_point": 60, "rows": rows}


def _queue(args, model, distinct: bool, n_requests: int, budgets):
    import torch
    from visualcla.synthetic import make_inputs
    n_img = n_requests if distinct else args.images
    prompts, image_of, _ = bench_prompts(n_img, n_requests // n_img, False, args.seed)
    px, _, _ = make_inputs(model.config, n_img, 128)
    px = px.to(model.device, torch.bfloat16)
    ids = torch.tensor(prompts, device=model.device)
    # a new pixel tensor per request, as chat_many builds them: sharing has to find equal images by value
    return [dict(input_ids=ids[i], pixel_values=px[image_of[i]].clone(), max_new_tokens=budgets[i]) for i in range(n_requests)]


def _queue_leg(args, distinct: bool) -> dict:
    import torch
    model = _model(args)
    B, N = args.slots, args.requests
    b = budgets_of(args.seed, N)
    reqs = _queue(args, model, distinct, N, b)
    kw = dict(do_sample=False, eos_token_id=None, max_batch=B, steps_per_sync=args.steps_per_sync)

    def run(share):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = model.generate_many(reqs, share_prefix=share, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert [len(x) for x in got] == b
        st = model.last_inflight_stats
        return got, {"s": round(dt, 3), "tok_s": round(sum(b) / dt, 1), "admission_s": round(st["admission_s"], 3), "steps_s": round(st["steps_s"], 3),
                     "steps": st["steps"], **{k: st[k] for k in ("rows_reused", "rows_computed", "vision_runs", "pool_entries", "pool_bytes", "admission_passes",
                                                                 "rows_calls", "workspace_bytes") if k in st}}
    for share in (False, True):                                  # warm-up: every shape of the timed windows once (code objects, graphs, workspaces)
        model.generate_many([dict(r, max_new_tokens=9 + (k % 3)) for k, r in enumerate(reqs[:B + 8])], share_prefix=share, **kw)
    takes = []
    agree = None
    for _ in range(2):                                           # two takes, the legs alternating
        off_toks, off = run(False)
        on_toks, on = run(True)
        takes.append({"off": off, "on": on})
        agree = sum(int(torch.equal(x, y)) for x, y in zip(off_toks, on_toks))
    off_spread = abs(takes[0]["off"]["s"] - takes[1]["off"]["s"])
    adm_spread = abs(takes[0]["off"]["admission_s"] - takes[1]["off"]["admission_s"])
    best = {k: min(t[k]["s"] for t in takes) for k in ("off", "on")}
    best_adm = {k: min(t[k]["admission_s"] for t in takes) for k in ("off", "on")}
    return {"leg": "queue_b" if distinct else "queue_a", "requests": N, "slots": B, "images": N if distinct else args.images, "budgeted_tokens": sum(b),
            "takes": takes, "off_spread_s": round(off_spread, 3), "off_admission_spread_s": round(adm_spread, 3), "best_s": best, "best_admission_s": best_adm,
            "on_over_off": round(best["on"] / best["off"], 4), "requests_with_equal_ids_on_and_off": agree,
            "note": "bf16: copied and computed rows come from differently tiled passes, so ids may part at near-ties (DESIGN.md 7e)"}


def leg_queue_a(args) -> dict:
    return _queue_leg(args, False)


def leg_queue_b(args) -> dict:
    return _queue_leg(args, True)


def leg_admission(args) -> dict:
    """one boundary: 64 requests with budget 1 (every request ends at its first token: generate_many is admission alone) -- 16 questions x 4 images"""
    import torch
    model = _model(args)
    B = args.slots
    n_img = 4
    prompts, image_of, _ = bench_prompts(n_img, B // n_img, False, args.seed)
    from visualcla.synthetic import make_inputs
    px, _, _ = make_inputs(model.config, n_img, 128)
    px = px.to(model.device, torch.bfloat16)
    ids = torch.tensor(prompts, device=model.device)
    reqs = [dict(input_ids=ids[i], pixel_values=px[image_of[i]].clone(), max_new_tokens=1) for i in range(B)]
    kw = dict(do_sample=False, eos_token_id=None, max_batch=B)

    def run(share):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate_many(reqs, share_prefix=share, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000
    for share in (False, True, False, True):
        run(share)
    takes = []
    for _ in range(2):
        ms = {"off": [], "on": []}
        for _ in range(3):
            ms["off"].append(run(False))
            ms["on"].append(run(True))
        takes.append({k: round(min(v), 3) for k, v in ms.items()})
    st = dict(model.last_inflight_stats)
    # the split of the `on` side, in a run of its own: a synchronise around the vision stack, the pool copies and the rows pass
    parts = {"vision": 0.0, "rows_pass": 0.0}
    orig_img, orig_rows = model.embed_images, model._extend_rows

    def timed(name, fn):
        def inner(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            parts[name] += (time.perf_counter() - t0) * 1000
            return out
        return inner
    model.embed_images, model._extend_rows = timed("vision", orig_img), timed("rows_pass", orig_rows)
    try:
        total = run(True)
    finally:
        model.embed_images, model._extend_rows = orig_img, orig_rows
    parts = {k: round(v, 3) for k, v in parts.items()}
    parts["plan_copies_and_host"] = round(total - sum(parts.values()), 3)
    return {"leg": "admission", "requests": B, "images": n_img, "ms_take1": takes[0], "ms_take2": takes[1],
            "off_spread_ms": round(abs(takes[0]["off"] - takes[1]["off"]), 3), "rows_reused": st["rows_reused"], "rows_computed": st["rows_computed"],
            "vision_runs": st["vision_runs"], "passes": st["admission_passes"], "on_split_ms_synchronised_run": dict(parts, total=round(total, 3))}


LEGS = {"kernel": leg_kernel, "admission": leg_admission, "queue_a": leg_queue_a, "queue_b": leg_queue_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--steps-per-sync", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--leg", choices=sorted(LEGS), help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--legs", default="kernel,admission,queue_a,queue_b", help="the legs the parent runs, in order")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.normpath(os.path.join(ROOT, "profiles", "prefix_sharing.txt")), help="rewritten with one line per leg run")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(LEGS[args.leg](args)), flush=True)
        return 0
    lines = [json.dumps(prediction(args))]
    print(lines[0], flush=True)
    if args.predict_only:
        return 0
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg] + \
              [x for k in ("requests", "slots", "images", "steps_per_sync", "seed", "layers") for x in (f"--{k.replace('_', '-')}", str(getattr(args, k)))]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                    # nothing more is started on the GPU after a failed leg
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"prefix_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/prefix_probe.py on MI355X: one JSON line per leg (prediction: host arithmetic; kernel, admission, queue_a, queue_b: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

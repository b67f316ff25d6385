"""Per-request token constraints at the full 7B shape (synthetic weights as bench.py builds them, bf16): what the mask and the transition of
csrc/constrain.hip add to a slots step, and what a queue of multiple-choice questions costs as constrained requests against scoring every
candidate with `target_ids`.

    python tools/constrain_probe.py [--requests 256] [--slots 64] [--prompt 128] [--steps-per-sync 8] [--seed 0] [--out profiles/constrained_decoding.txt]

The parent process never touches the GPU: it prints the table sizes and the bytes per step (host arithmetic), then runs every GPU leg as a
child process under a time limit of its own and stops at the first leg that fails.  Every leg prints one JSON line; the parent writes them
to --out.

    step_cost   ms per graph-replayed slots step at B = slots, all slots active: no constraints / every row under a 4-id allow list / a 4-id
                deny list / a 12-choice trie (its eos edges lead back to the root, so the rows keep walking it), each on the argmax path and
                on the sampler path (the reference's default sampling config), and the allow list again beside logprobs=5; alternating in
                one process, `--rounds` takes each.  Condition: a constrained step costs at most 1.05 x the unconstrained step of the same
                run and path (the margin of DESIGN.md sections 7f, 7g and 7h)
    queue       the inflight_probe queue with every request under four choices of 1-3 tokens, against the same questions answered by
                scoring the four candidates with target_ids (4 x requests forced requests, logprobs=0), with and without share_prefix
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

from inflight_probe import _model  # noqa: E402

PARENT_STEP_MS = {"argmax": 4.5282, "sampler": 4.5685}      # profiles/logprobs.txt, step_cost (ms_per_step_min, logprobs None)
PARENT_SPREAD_MS = (0.003, 0.006)                            # the same file: the spread of its takes
VOCAB = 49958
EOS = 2
KINDS = ("none", "allow4", "deny4", "trie12")


def _specs(kind, B, seed=0):
    """the constraint of every row for one variant (None: unconstrained)"""
    from visualcla import constraints as K
    rng = random.Random(seed)
    if kind == "none":
        return [None] * B
    if kind in ("allow4", "deny4"):
        return [K.parse(b, {"allowed_token_ids" if kind == "allow4" else "banned_token_ids": [1000, 1001, 20000, 49000]}) for b in range(B)]
    firsts = rng.sample(range(3, VOCAB - 8), 6)                  # twelve choices of 1-3 tokens over six first tokens: shared prefixes
    choices = [[firsts[k % 6]] + rng.sample(range(3, VOCAB - 8), k % 3) for k in range(12)]
    return [K.parse(b, {"choices": choices}) for b in range(B)]


def prediction(args) -> dict:
    from visualcla import constraints as K
    B = args.slots
    row = VOCAB * 4
    tables = {}
    for kind in KINDS[1:]:
        tb = K.build(_specs(kind, B), [[EOS]] * B)
        tables[kind] = dict(tb.stats(), automata=tb.automata, table_bytes=16 * len(tb.nodes) + 8 * len(tb.edges), state_bytes=4 * B)
    return {"leg": "prediction", "slots": B, "vocab": VOCAB, "tables": tables, "bitmask_lds_bytes": (VOCAB + 31) // 32 * 4,
            "mask_write_bytes_allow4": B * (row - 16), "mask_write_bytes_deny4": B * 16, "issue_expectation_bytes": {"read": B * row, "write": B * row},
            "parent_step_ms": PARENT_STEP_MS,
            "note": "the issue expected one more read and write of the 12.8 MB of rows; the kernel never reads the row (a kept column is simply not "
                    "written), so an allow list writes 12.8 MB of -inf and a deny list 16 bytes per row, against a step of ~4.5 ms: under 1 % by "
                    "bytes; the pass is one workgroup per row, so its time is that workgroup's stores and two barriers, not bandwidth"}


def leg_step_cost(args) -> dict:
    import torch
    from visualcla import _lib
    from visualcla import constraints as K
    model = _model(args)
    lib = _lib.load()
    dev = model.device
    t = model.config.text_config
    B, T, n = args.slots, args.prompt, args.steps
    V = t["vocab_size"]
    ctx_max = (T + n + 2 + 63) // 64 * 64
    H, d = t["num_attention_heads"], t["hidden_size"] // t["num_attention_heads"]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        kv = (torch.randn(t["num_hidden_layers"], 2, B, H, ctx_max, d, device=dev) * 0.3).to(torch.bfloat16)
        km = torch.ones(B, ctx_max, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.vcla_llama_workspace_bytes(model._ctx, B, 1) + lib.vcla_logprob_scratch_bytes(B, V, 1) + 512, dtype=torch.uint8, device=dev)
        ids = torch.randint(3, V - 8, (B,), generator=torch.Generator().manual_seed(3)).to(dev)
        W = _lib.SLOT_SUMMARY_WORDS
        cap = n + 2
        st = torch.zeros(4 * B + W, dtype=torch.int32, device=dev)
        hist = torch.zeros(cap, B, dtype=torch.int64, device=dev)
        uni = torch.rand(cap, B, device=dev)
        cur = ids.clone()
        slots = _lib.slot_args([], st[:B], st[B:2 * B], st[3 * B:4 * B], st[2 * B:3 * B], hist, cur, st[4 * B:])
        init = torch.tensor([T] * B + [1] * B + [1] * B + [cap] * B + [0] * W, dtype=torch.int32, device=dev)
        samp = _lib.sample_args(uniforms=uni, history=hist, repetition_penalty=1.1, no_repeat_ngram_size=15, temperature=0.5, top_k=40, top_p=0.9)
        tok_lp = torch.zeros(cap, B, dtype=torch.float32, device=dev)
        top_ids = torch.zeros(cap, B, 5, dtype=torch.int64, device=dev)
        top_lp = torch.zeros(cap, B, 5, dtype=torch.float32, device=dev)
        lp5 = _lib.logprob_args(5, tok_lp, top_ids, top_lp)
        cons, keep_alive, roots = {}, [], {}
        for kind in KINDS[1:]:
            tb = K.build(_specs(kind, B), [[EOS]] * B)
            if kind == "trie12":                                 # no row ever ends here: the eos edges lead back to the root and the rows keep walking
                for e in tb.edges:
                    if e[0] == EOS:
                        e[1] = tb.roots[0]
            nodes, edges = tb.tensors(dev)
            state = torch.zeros(B, dtype=torch.int32, device=dev)
            keep_alive.append((nodes, edges))
            roots[kind] = (state, torch.tensor(tb.roots, dtype=torch.int32, device=dev))
            cons[kind] = _lib.constrain_args(nodes, edges, state)

        def run(path, kind, lp, steps):
            st.copy_(init)
            cur.copy_(ids)
            if kind != "none":
                roots[kind][0].copy_(roots[kind][1])
            _lib.check(lib.vcla_llama_decode_slots_constrained(model._ctx, C.byref(slots), steps, kv.data_ptr(), ctx_max, km.data_ptr(), ws.data_ptr(), ws.numel(), 1,
                                                               C.byref(samp) if path == "sampler" else None, None, None, C.byref(lp5) if lp else None,
                                                               C.byref(cons[kind]) if kind != "none" else None, _lib.stream_ptr()))

        def timed(path, kind, lp):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run(path, kind, lp, 1)                               # one graph slot, alternating keys: the capture happens here, untimed
            e0.record(stream)
            run(path, kind, lp, n)
            e1.record(stream)
            torch.cuda.synchronize()
            assert st[4 * B].item() == B and st[:B].tolist() == [T + n] * B, "every slot must still be active"
            return e0.elapsed_time(e1) / n
        variants = [(p, k, 0) for p in ("argmax", "sampler") for k in KINDS] + [(p, k, 5) for p in ("argmax", "sampler") for k in ("none", "allow4")]
        name = lambda p, k, lp: f"{p}/{k}" + ("+logprobs5" if lp else "")      # noqa: E731
        checks = {}
        for p, k, lp in variants:                                # warm-up: code objects; and that the constraint holds in what the rows took
            run(p, k, lp, 8)
            torch.cuda.synchronize()
            taken = hist[1:9].cpu()
            if k == "allow4":
                checks[name(p, k, lp)] = bool(torch.isin(taken, torch.tensor([1000, 1001, 20000, 49000, 0])).all())     # (0: a row the n-gram ban emptied)
            elif k == "deny4":
                checks[name(p, k, lp)] = not bool(torch.isin(taken, torch.tensor([1000, 1001, 20000, 49000])).any())
            elif k == "trie12":
                checks[name(p, k, lp)] = len(set(roots[k][0].tolist())) > 1      # the rows are spread over the trie's nodes
        ms = {name(*v): [] for v in variants}
        for _ in range(args.rounds):                             # alternating
            for v in variants:
                ms[name(*v)].append(timed(*v))
    best = {k: min(v) for k, v in ms.items()}
    ratio = {k: round(v / best[k.split("/")[0] + "/none" + ("+logprobs5" if k.endswith("+logprobs5") else "")], 4) for k, v in best.items() if "/none" not in k}
    none_vs_parent = {p: round(best[f"{p}/none"] / PARENT_STEP_MS[p], 4) for p in ("argmax", "sampler")}
    return {"leg": "step_cost", "B": B, "context": f"{T}..{T + n}", "steps_per_sample": n, "samples_each": args.rounds,
            "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "ms_per_step_min": {k: round(v, 4) for k, v in best.items()},
            "constrained_over_unconstrained": ratio, "condition": "every constrained step <= 1.05 x the unconstrained step of the same run, path and logprobs",
            "condition_met": bool(max(ratio.values()) <= 1.05), "none_over_parent_step": none_vs_parent,
            "none_minus_parent_ms": {p: round(best[f"{p}/none"] - PARENT_STEP_MS[p], 4) for p in ("argmax", "sampler")}, "parent_step_ms": PARENT_STEP_MS,
            "parent_spread_ms": PARENT_SPREAD_MS, "constraints_hold_in_the_tokens_taken": checks,
            "note": "variant = path/constraint of all 64 rows; every timed window replays a captured step; sampler = the reference's default sampling config"}


def leg_queue(args) -> dict:
    import torch
    from visualcla.synthetic import make_inputs
    model = _model(args)
    B, T, N = args.slots, args.prompt, args.requests
    rng = random.Random(args.seed)
    px, ids, _ = make_inputs(model.config, N, T)
    px, ids = px.to(model.device, torch.bfloat16), ids.to(model.device)
    choices = [[rng.sample(range(3, VOCAB - 8), 1 + (i + k) % 3) for k in range(4)] for i in range(N)]      # four choices of 1-3 tokens per request
    cons = [dict(input_ids=ids[i], pixel_values=px[i], max_new_tokens=8, choices=choices[i]) for i in range(N)]
    forced = [dict(input_ids=ids[i], pixel_values=px[i], target_ids=c) for i in range(N) for c in choices[i]]
    kw = dict(max_batch=B, steps_per_sync=args.steps_per_sync, do_sample=False, eos_token_id=EOS)

    def go(rs, **extra):
        t0 = time.perf_counter()
        o = model.generate_many(rs, **kw, **extra)
        torch.cuda.synchronize()
        return o, time.perf_counter() - t0, dict(model.last_inflight_stats)
    go(cons[:B + 8])                                             # warm-up: every route once (code objects, graphs)
    go(forced[:B + 8], logprobs=0)
    go(forced[:B + 8], logprobs=0, share_prefix=True)
    out, t_cons, st_cons = go(cons)
    ok = sum(o.tolist()[:-1] in choices[i] and int(o[-1]) == EOS for i, o in enumerate(out))
    useful = sum(int(o.numel()) for o in out)
    scored, t_forced, st_forced = go(forced, logprobs=0)
    scored_sh, t_forced_sh, st_forced_sh = go(forced, logprobs=0, share_prefix=True)
    best = [max(range(4), key=lambda k: float(scored[4 * i + k].logprobs.sum())) for i in range(N)]
    agree = sum(out[i].tolist()[:-1] == choices[i][best[i]] for i in range(N))
    return {"leg": "queue", "requests": N, "slots": B, "prompt": T, "choices_per_request": 4,
            "constrained": {"s": round(t_cons, 3), "useful_tokens": useful, "useful_tok_s": round(useful / t_cons, 1), "requests_s": round(N / t_cons, 1),
                            "steps": st_cons["steps"], "admission_s": round(st_cons["admission_s"], 3), "steps_s": round(st_cons["steps_s"], 3),
                            "automaton_nodes": st_cons["automaton_nodes"], "automaton_edges": st_cons["automaton_edges"], "outputs_that_are_a_choice_plus_eos": ok},
            "scored_with_target_ids": {"forced_requests": len(forced), "s": round(t_forced, 3), "questions_s": round(N / t_forced, 1), "steps": st_forced["steps"],
                                       "admission_s": round(st_forced["admission_s"], 3), "steps_s": round(st_forced["steps_s"], 3)},
            "scored_with_target_ids_share_prefix": {"s": round(t_forced_sh, 3), "questions_s": round(N / t_forced_sh, 1), "steps": st_forced_sh["steps"],
                                                    "admission_s": round(st_forced_sh["admission_s"], 3), "steps_s": round(st_forced_sh["steps_s"], 3)},
            "constrained_over_scored": round(t_cons / t_forced, 4), "constrained_over_scored_share_prefix": round(t_cons / t_forced_sh, 4),
            "greedy_walk_equals_best_summed_logprob": agree,
            "note": "a report, not a condition.  A greedy walk of the trie and the candidate of the largest summed log-probability are different "
                    "decision rules: they need not agree"}


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
    ap.add_argument("--out", default=os.path.join("profiles", "constrained_decoding.txt"))
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
            print(f"constrain_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/constrain_probe.py on MI355X: one JSON line per leg (prediction: host arithmetic; step_cost, queue: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

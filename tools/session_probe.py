"""Chat sessions at the full 7B shape (synthetic weights as bench.py builds them, bf16, one image): what the later-turn attention kernel, the
later-turn decoder block and a whole scripted conversation cost next to what the same work costs without a session.

    python tools/session_probe.py [--turns 6] [--new 24] [--gen 64] [--reps 5] [--layers 0] [--out profiles/sessions.txt]

The parent process never touches the GPU: it prints the prediction (host arithmetic: rows computed per turn with and without a session,
K/V bytes the attention walks), then runs every GPU leg as a child process under a time limit of its own and stops at the first leg that
fails.  Every leg prints one JSON line; the parent writes them to --out.

    kernel   vcla_attn_extend against vcla_rope_kv_append + vcla_attention (what vcla_llama_prefill(pos0 = P) launches) and, for R <= 16,
             vcla_attn_verify: us per layer, alternating, >= 200 launches per point; K/V bytes walked over time as a share of the HBM peak;
             the outputs of the forms compared at the timed sizes (atol 1.6e-2).  The table is taken twice for the spread.
    block    vcla_llama_extend against vcla_llama_prefill(pos0 = P) at P = 600: ms per call (host clock around a synchronise), the prefill
             both as a conversation meets it (a new (T, pos0) every turn: eager launches) and replayed from its captured graph
    turns    a scripted conversation (turn k: the previous prompt + its `gen` generated tokens + `new` prompt tokens): per turn the time to
             first token (generate(max_new_tokens=1)) and the whole turn, with and without a session, alternating
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

HBM_PEAK = 8.0e12           # bytes/s (MI355X_MICROARCH: HBM3E)
RS = (8, 16, 24, 64, 128, 256)
PS = (200, 600, 1200, 1900)
H, D, CTX = 32, 128, 2048


def prediction(args) -> dict:
    first = 128
    rows = []
    for k in range(args.turns):
        T = first + k * (args.gen + args.new)
        P = 0 if k == 0 else T - args.new - 1          # the prompt and all but the last generated token have rows
        rows.append({"turn": k + 1, "prompt": T, "rows_without": T, "rows_with": T - P, "kv_mib_walked_per_layer": round(2 * H * T * D * 2 / 2 ** 20, 2)})
    return {"leg": "prediction", "turns": rows}


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


def leg_kernel(args) -> dict:
    import torch
    from visualcla import _lib
    from visualcla.weights import rope_tables
    _lib.require_device()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    cos, sin = (t.to(dev) for t in rope_tables(CTX, D, 10000.0))
    kv = (torch.randn(2, H, CTX, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    scale = D ** -0.5
    stream = torch.cuda.Stream(device=dev)
    tables = []
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for _ in range(2):
            table = []
            for R in RS:
                for P in PS:
                    if P + R > CTX:
                        continue
                    qkv0 = torch.randn(R, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
                    qkv = qkv0.clone()
                    out_x = torch.zeros(R, H * D, dtype=torch.bfloat16, device=dev)
                    out_p, out_v = torch.zeros_like(out_x), torch.zeros_like(out_x)
                    nb = lib.vcla_attn_extend_scratch_bytes(R, H, D, P)
                    sx = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
                    sv = torch.empty(max(lib.vcla_attn_verify_scratch_bytes(H, D, CTX), 16), dtype=torch.uint8, device=dev)
                    a = _lib.AttnArgs()
                    a.q, a.k, a.v, a.o = qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), out_p.data_ptr()
                    a.q_bs, a.q_hs, a.q_rs = R * 3 * H * D, D, 3 * H * D
                    a.k_bs = a.v_bs = H * CTX * D
                    a.k_hs = a.v_hs = CTX * D
                    a.k_rs = a.v_rs = D
                    a.o_bs, a.o_hs, a.o_rs = R * H * D, D, H * D
                    a.B, a.H, a.Tq, a.Tk, a.D, a.scale, a.causal = 1, H, R, P + R, D, scale, 1

                    def extend():
                        _lib.check(lib.vcla_attn_extend(qkv0.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_x.data_ptr(), R, H, D,
                                                        CTX, P, scale, _lib.VCLA_BF16, 0, sx.data_ptr(), sx.numel(), _lib.stream_ptr()))

                    def pair():
                        _lib.check(lib.vcla_rope_kv_append(qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), 1, R, H, D, CTX, P,
                                                           None, _lib.VCLA_BF16, _lib.stream_ptr()))
                        _lib.check(lib.vcla_attention(C.byref(a), _lib.VCLA_BF16, _lib.stream_ptr()))

                    def verify():
                        _lib.check(lib.vcla_attn_verify(qkv0.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), cos.data_ptr(), sin.data_ptr(), out_v.data_ptr(), R, H, D,
                                                        CTX, P, None, None, scale, _lib.VCLA_BF16, 0, sv.data_ptr(), sv.numel(), _lib.stream_ptr()))
                    forms = {"extend": extend, "pair": pair}
                    if R <= 16:
                        forms["verify"] = verify
                    # the outputs at this size, from one qkv (the pair rotates its copy in place: compared on the first call only)
                    for fn in forms.values():
                        fn()
                    torch.cuda.synchronize()
                    diff = {k: float((o.float() - out_x.float()).abs().max()) for k, o in (("pair", out_p), ("verify", out_v)) if k in forms}
                    assert all(v <= 1.6e-2 for v in diff.values()), (R, P, diff)
                    for fn in forms.values():                    # warm-up
                        for _ in range(10):
                            fn()
                    us = {k: [] for k in forms}
                    for _ in range(4):                           # alternating, 4 x 50 launches per form
                        for k, fn in forms.items():
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            for _ in range(50):
                                fn()
                            e1.record(stream)
                            torch.cuda.synchronize()
                            us[k].append(e0.elapsed_time(e1) * 1000 / 50)
                    best = {k: round(min(v), 2) for k, v in us.items()}
                    walked = 2 * H * (P + R) * D * 2
                    table.append({"R": R, "P": P, "us": best, "extend_share_of_hbm_peak": round(walked / (best["extend"] * 1e-6) / HBM_PEAK, 4),
                                  "max_abs_diff_vs_extend": {k: round(v, 5) for k, v in diff.items()}})
            tables.append(table)
    spread = max(abs(x["us"][k] - y["us"][k]) / min(x["us"][k], y["us"][k]) for x, y in zip(*tables) for k in x["us"])
    return {"leg": "kernel", "H": H, "d": D, "ctx_max": CTX, "launches_per_point": 200, "tables": tables, "largest_relative_spread_between_tables": round(spread, 4)}


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000


def leg_block(args) -> dict:
    import torch
    from visualcla.modeling_visualcla import VclaCache
    model = _model(args)
    dev = model.device
    t = model.config.text_config
    P = 600
    stream = torch.cuda.Stream(device=dev)
    rows = []
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        ids = torch.randint(3, 30000, (1, P + 1 + 128), generator=torch.Generator().manual_seed(1)).to(dev)
        emb, _ = model._embed(ids, None, None)
        cache = VclaCache(torch.empty(t["num_hidden_layers"], 2, 1, H, CTX, D, dtype=torch.bfloat16, device=dev), 0, CTX)
        model._prefill(emb[:, :P + 1].contiguous(), cache, None, all_logits=False)
        for T in (8, 24, 64, 65, 128):
            x0, x1 = emb[:, P:P + T].contiguous(), emb[:, P + 1:P + 1 + T].contiguous()
            flip = [0]

            def extend():
                cache.length = P
                model._extend(x0, cache)

            def prefill_eager():                               # a new (T, pos0) on every call, as the turns of a conversation present it
                flip[0] ^= 1
                cache.length = P + flip[0]
                model._prefill(x1 if flip[0] else x0, cache, None, all_logits=False)

            def prefill_replay():                              # the same call again: replayed from the prefill's captured graph
                cache.length = P
                model._prefill(x0, cache, None, all_logits=False, _persistent=True)
            forms = {"extend": extend, "prefill_eager": prefill_eager, "prefill_replay": prefill_replay}
            for fn in forms.values():
                for _ in range(3):
                    fn()
            ms = {k: [] for k in forms}
            for _ in range(args.reps * 2):
                for k, fn in forms.items():
                    ms[k].append(_timed(torch, fn))
            rows.append({"T": T, "P": P, "ms_min": {k: round(min(v), 3) for k, v in ms.items()}, "ms_median": {k: round(sorted(v)[len(v) // 2], 3) for k, v in ms.items()}})
    return {"leg": "block", "layers": t["num_hidden_layers"], "samples_each": args.reps * 2, "rows": rows}


def leg_turns(args) -> dict:
    import torch
    from visualcla.synthetic import make_inputs
    model = _model(args)
    dev = model.device
    px, ids, _ = make_inputs(model.config, 1, 128)
    px = px.to(dev, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    kw = dict(do_sample=False, eos_token_id=None, pixel_values=px)
    per_turn = [{"turn": k + 1, "ttft_with": [], "ttft_without": [], "turn_with": [], "turn_without": []} for k in range(args.turns)]
    new_ids = [torch.randint(3, 30000, (1, args.new), generator=g) for _ in range(args.turns)]
    for rep in range(args.reps + 1):                             # repetition 0 warms every shape up and is dropped
        s = model.new_session()
        prompt = ids.clone()
        for k in range(args.turns):
            p = prompt.to(dev)
            held = list(s.ids)
            order = ("with", "without") if (rep + k) % 2 == 0 else ("without", "with")
            rec = {}
            for which in order:
                extra = {"session": s} if which == "with" else {}
                rec["ttft_" + which] = _timed(torch, lambda: model.generate(input_ids=p, max_new_tokens=1, **extra, **kw))
                if which == "with":
                    stats = dict(model.last_session_stats)
                    s.ids = held                                 # the whole turn starts from the rows the session held before this turn
                out = []
                rec["turn_" + which] = _timed(torch, lambda: out.append(model.generate(input_ids=p, max_new_tokens=args.gen, **extra, **kw)))
                if which == "with":
                    toks = out[0].cpu()
            if rep:
                for key, v in rec.items():
                    per_turn[k][key].append(round(v, 3))
                per_turn[k].update(prompt=int(prompt.shape[1]), reused=stats["reused"], prefilled=stats["prefilled"], vision_skipped=stats["vision_skipped"])
            prompt = torch.cat([prompt, toks, new_ids[k]], dim=1)
        del s
    for r in per_turn:
        for key in ("ttft_with", "ttft_without", "turn_with", "turn_without"):
            r[key + "_min"] = min(r[key])
        r["decode_with_min"] = round(r["turn_with_min"] - r["ttft_with_min"], 3)
    return {"leg": "turns", "new": args.new, "gen": args.gen, "reps": args.reps, "session_mib": round(model.new_session().nbytes / 2 ** 20, 1),
            "row_copy_ms": 0.0, "per_turn": per_turn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=6)
    ap.add_argument("--new", type=int, default=24)
    ap.add_argument("--gen", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0, help="text layers (0: the full 32)")
    ap.add_argument("--leg", choices=["kernel", "block", "turns"], help="run ONE GPU leg in this process (what the parent spawns)")
    ap.add_argument("--legs", default="kernel,block,turns")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds per GPU leg")
    ap.add_argument("--predict-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "sessions.txt"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps({"kernel": leg_kernel, "block": leg_block, "turns": leg_turns}[args.leg](args)), flush=True)
        return 0
    lines = [json.dumps(prediction(args))]
    print(lines[0], flush=True)
    if args.predict_only:
        return 0
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg] + \
              [x for k in ("turns", "new", "gen", "reps", "layers") for x in (f"--{k}", str(getattr(args, k)))]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                                    # nothing more is started on the GPU after a failed leg
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"session_probe: leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line[:3000], flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/session_probe.py on MI355X: one JSON line per leg (prediction: host arithmetic; kernel, block, turns: measured)\n")
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

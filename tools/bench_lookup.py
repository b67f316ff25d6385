"""Prompt-lookup decoding at the full 7B shape (synthetic weights, VisualCLAModel.from_random): the cost of one verify iteration against one plain
decode step, and end-to-end greedy generation with and without prompt_lookup_num_tokens on a prompt built to repeat.  Prints one JSON line.

    python tools/bench_lookup.py [--prompt 128] [--iters 32] [--new 128]

Break-even: a verify iteration at k drafts costs t_verify(k); it emits 1 + (accepted drafts) tokens, a plain step emits 1 in t_engine.  The
lookup path wins when the accepted drafts per iteration exceed t_verify(k) / t_engine - 1.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "visual-chinese-llama-alpaca_amd"))
import visualcla  # noqa: E402
from visualcla import _lib  # noqa: E402
from visualcla.synthetic import stub_tokenizer  # noqa: E402


def _time(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def plain_step_ms(model, T, n_steps):
    lib = _lib.load()
    V = model.config.text_config["vocab_size"]
    ids = torch.randint(3, V - 8, (1, T), generator=torch.Generator().manual_seed(11)).to(model.device)
    ctx_max = (T + n_steps + 2 + 63) // 64 * 64
    embeds, _ = model._embed(ids, None, None)
    stream = torch.cuda.Stream(device=model.device)
    with torch.cuda.stream(stream):
        cache = model._new_cache(1, ctx_max, _persistent=True)
        model._prefill(embeds, cache, None, all_logits=False, _persistent=True)
        ws = model._buf("llama", lib.vcla_llama_workspace_bytes(model._ctx, 1, 1))
        out = model._typed_buf("gen_out", (n_steps + 1, 1), torch.int64)
        out[0] = 17

        def loop():
            model._pos_dev.zero_()
            _lib.check(lib.vcla_llama_decode_loop(model._ctx, out[0].data_ptr(), 1, T, model._pos_dev.data_ptr(), n_steps, cache.kv.data_ptr(), ctx_max,
                                                  None, out[1:].data_ptr(), ws.data_ptr(), ws.numel(), 1, _lib.stream_ptr()))
        loop()
        torch.cuda.synchronize()
        sec = _time(loop, stream) / n_steps
        _lib.check(lib.vcla_llama_decode_status(model._ctx, 1, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    return sec * 1e3


def verify_iter_ms(model, k, T, iters):
    """iters replayed verify iterations (no eos, a budget that never runs out) after one warm-up iteration that captures the graph"""
    lib = _lib.load()
    dev = model.device
    V = model.config.text_config["vocab_size"]
    ids = torch.randint(3, V - 8, (1, T), generator=torch.Generator().manual_seed(12)).to(dev)
    budget = (iters + 1) * (k + 1) + 2
    ctx_max = min(model.config.text_config["max_position_embeddings"], (T + budget + k + 63) // 64 * 64)
    embeds, _ = model._embed(ids, None, None)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        cache = model._new_cache(1, ctx_max)
        model._prefill(embeds, cache, None, all_logits=False)
        hist = torch.zeros(T + budget, dtype=torch.int64, device=dev)
        hist[:T] = ids[0]
        hist[T] = 17
        out = torch.zeros(budget, dtype=torch.int64, device=dev)
        out[0] = 17
        row = torch.zeros(k + 1, dtype=torch.int64, device=dev)
        state = torch.zeros(_lib.LOOKUP_STATE_WORDS, dtype=torch.int32, device=dev)
        state[_lib.LOOKUP_NHIST], state[_lib.LOOKUP_COUNT] = T + 1, 1
        model._pos_dev.zero_()
        a = _lib.lookup_args(k, 2, budget, [], row, hist, out, state)
        ws = model._buf("lookup", lib.vcla_llama_verify_workspace_bytes(model._ctx, ctx_max))
        _lib.check(lib.vcla_lookup_step(None, C.byref(a), model._pos_dev.data_ptr(), _lib.stream_ptr()))

        def run(n):
            _lib.check(lib.vcla_llama_verify_loop(model._ctx, C.byref(a), T, model._pos_dev.data_ptr(), n, cache.kv.data_ptr(), ctx_max, None,
                                                  ws.data_ptr(), ws.numel(), 1, _lib.stream_ptr()))
        run(1)
        torch.cuda.synchronize()
        sec = _time(lambda: run(iters), stream) / iters
        st = state.tolist()
    assert not st[_lib.LOOKUP_DONE]
    return sec * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--new", type=int, default=128)
    args = ap.parse_args()
    cfg = visualcla.visualcla_7b_config()
    model = visualcla.VisualCLAModel.from_random(cfg, device=torch.device("cuda", 0), torch_dtype=torch.bfloat16, seed=0)
    model.tokenizer = stub_tokenizer()
    model.image_at_head = False
    res = {"tool": "bench_lookup", "shape": "LLaMA-7B text decoder (32 layers, hidden 4096), synthetic weights, bf16, B = 1", "prompt": args.prompt}
    t_eng = plain_step_ms(model, args.prompt, 64)
    res["plain_step_ms"] = round(t_eng, 4)
    res["verify_iter_ms"] = {}
    res["break_even_accepted_per_iter"] = {}
    for k in (1, 2, 4, 7, 15):
        t = verify_iter_ms(model, k, args.prompt, args.iters)
        res["verify_iter_ms"][str(k)] = round(t, 4)
        res["break_even_accepted_per_iter"][str(k)] = round(t / t_eng - 1.0, 3)
    # end to end on a prompt built to repeat: a phrase of 16 ids, 8 times
    V = model.config.text_config["vocab_size"]
    g = torch.Generator().manual_seed(5)
    phrase = torch.randint(3, V - 8, (16,), generator=g)
    ids = torch.cat([torch.randint(3, V - 8, (args.prompt - 128,), generator=g), phrase.repeat(8)])[None].to(model.device)
    kw = dict(input_ids=ids, max_new_tokens=args.new, do_sample=False, eos_token_id=None)
    model.generate(**kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plain = model.generate(**kw)
    torch.cuda.synchronize()
    t_plain = time.perf_counter() - t0
    e2e = {"plain_tok_s": round(args.new / t_plain, 1)}
    for k in (2, 4, 7):
        model.generate(prompt_lookup_num_tokens=k, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        look = model.generate(prompt_lookup_num_tokens=k, **kw)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        st = model.last_lookup_stats
        e2e[f"k{k}"] = {"tok_s": round(args.new / t, 1), "iterations": st["iterations"], "accepted": st["accepted"],
                        "tokens_per_verify": round((st["tokens"] - 1) / max(st["iterations"], 1), 3), "ids_equal": bool(torch.equal(plain, look))}
    res["end_to_end_repetitive_prompt"] = e2e
    res["note"] = "tok/s include the prefill of the prompt; synthetic weights: acceptance here demonstrates the mechanism only"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

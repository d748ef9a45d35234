"""Prefill onto a live KV cache, measured in one process on one GPU at NVILA-8B widths with seeded synthetic weights.

  follow-up TTFT   turn 1 = the bench workload (one 448^2 image + 512 tokens, S = 769, 64 tokens generated); turn 2 adds 48 tokens.
                   (a) what `serving.ChatSession` runs: `prefill_append` of the 48 tokens onto the cache (the last emitted token among them);
                   (b) what the library had to do without it: encode the image again, splice, and prefill the whole conversation.
                   The same pair on a conversation of 2817 + 64 positions (the dynamic_s2 prompt's length; its embeddings are drawn, so (b) there
                   is the prefill alone, WITHOUT the tower pass it would also need).
  attention        per-launch time of the key-prefix attention at those two shapes, per form (vila_attn_force_append).
  chunked prefill  S = 2817 as prefill_chunk = 1024 against the one-shot prefill: time and workspace bytes.

    python tools/append_prefill_bench.py [--iters 7] [--layers 28] [--out profiles/append_prefill_bench.json]

Timing: HIP events around the calls on the current stream, warm (one untimed round first), arms alternating, median of `--iters` rounds.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vila_amd import _lib, configs, ops, synthetic  # noqa: E402

NEW_TOKENS, GENERATED = 48, 64
FORMS = {1: "A", 2: "B", 3: "C", 4: "D"}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(arms, iters):
    """arms: name -> callable.  One untimed round, then `iters` rounds with the arms in turn; -> name -> median ms."""
    ts = {k: [] for k in arms}
    for it in range(iters + 1):
        for k, fn in arms.items():
            t = timed(fn)
            if it:
                ts[k].append(t)
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}


def follow_up(model, e_prompt, re_embed, iters, tag):
    """Turn 1 on e_prompt [S, H], then the two ways to the first token of a 48-token turn 2."""
    llm, dev = model.llm, e_prompt.device
    S = e_prompt.shape[0]
    max_ctx = ((S + GENERATED + NEW_TOKENS + 64 + 255) // 256) * 256
    cache = llm.new_cache(max_ctx)
    out1 = llm.generate(inputs_embeds=e_prompt[None], max_new_tokens=GENERATED, eos_token_id=-1, cache=cache)[0]
    past = S + GENERATED - 1
    g = torch.Generator().manual_seed(S)
    turn2 = torch.randint(0, 30000, (NEW_TOKENS - 1,), generator=g).to(dev)
    e_new = llm.embed_tokens(torch.cat([out1[-1:], turn2])[None])[0]
    last_new = torch.full((1,), NEW_TOKENS - 1, device=dev, dtype=torch.int32)
    e_reply = llm.embed_tokens(out1[None])[0]
    whole_n = S + GENERATED + NEW_TOKENS - 1
    cache_b = llm.new_cache(max_ctx)
    pos_b = torch.arange(whole_n, device=dev, dtype=torch.int32)
    last_b = torch.full((1,), whole_n - 1, device=dev, dtype=torch.int32)

    def arm_a():
        llm.prefill_append(e_new, cache, past, 0, last_rows=last_new)

    def arm_b():
        whole = torch.cat([re_embed(), e_reply, e_new[1:]], 0)
        llm.prefill_packed(whole, pos_b, None, whole_n, cache=cache_b, last_rows=last_b)

    r = alternate({"append_ms": arm_a, "reprefill_ms": arm_b}, iters)
    form = _lib.load().vila_attn_append_form(NEW_TOKENS, llm.lcfg.num_attention_heads)
    r.update(case=tag, past=past, new_tokens=NEW_TOKENS, conversation=whole_n, append_attention_form=FORMS[form],
             speedup=round(r["reprefill_ms"] / r["append_ms"], 2))
    return r


def attention_launch(llm, past, iters, reps=20):
    """ms per launch of the key-prefix attention alone: T = 48 rows, the model's heads, per form."""
    lib, c = _lib.load(), llm.lcfg
    max_ctx = ((past + NEW_TOKENS + 255) // 256) * 256
    g = torch.Generator(device="cuda").manual_seed(past)
    q = torch.randn((NEW_TOKENS, c.num_attention_heads, 128), device="cuda", generator=g).to(torch.bfloat16)
    k = torch.randn((c.num_key_value_heads, max_ctx, 128), device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn((c.num_key_value_heads, max_ctx, 128), device="cuda", generator=g).to(torch.bfloat16)
    o = torch.empty_like(q)
    arms = {}
    for form, name in FORMS.items():
        def run(form=form):
            lib.vila_attn_force_append(form)
            for _ in range(reps):
                ops.attn_append(q, k, v, past, out=o)
        arms[name] = run
    try:
        r = alternate(arms, iters)
    finally:
        lib.vila_attn_force_append(0)
    return {"past": past, "T": NEW_TOKENS, "us_per_launch": {k: round(t * 1e3 / reps, 2) for k, t in r.items()}}


def chunked(llm, S, chunk, iters):
    lib, w = _lib.load(), llm._struct()
    g = torch.Generator(device="cuda").manual_seed(S)
    e = torch.randn((1, S, llm.lcfg.hidden_size), device="cuda", generator=g).mul_(0.02).to(torch.bfloat16)
    cache = llm.new_cache(((S + 8 + 255) // 256) * 256)
    arms = {"one_shot_ms": lambda: llm._prefill_one(e, None, 1, cache),
            "chunked_ms": lambda: llm._prefill_one(e, None, 1, cache, None, None, chunk)}
    r = alternate(arms, iters)
    r.update(S=S, chunk=chunk, one_shot_workspace_bytes=int(lib.vila_llm_prefill_workspace_bytes(C.byref(w.shape), S)),
             chunked_workspace_bytes=int(lib.vila_llm_prefill_append_workspace_bytes(C.byref(w.shape), chunk)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_prefill_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = a.layers
    model = build_model(cfg, seed=0)
    llm = model.llm
    with torch.inference_mode():
        px = synthetic.make_pixels(cfg, 1, 0, device="cuda", dtype=torch.bfloat16)
        ids = synthetic.make_prompt(cfg, 512, 1, 0)[None].cuda()
        embed = lambda: model._embed(ids, {"image": [px[0]]})[0][0]
        e769 = embed()
        res = {"config": {"model": cfg.name, "layers": a.layers, "timings": a.iters, "new_tokens": NEW_TOKENS, "generated_in_turn_1": GENERATED,
                          "method": "HIP events on the current stream, warm, arms alternating, median"}}
        res["follow_up"] = [follow_up(model, e769, embed, a.iters, "1 image + 512 tokens (S = 769): (b) re-encodes the image")]
        print(json.dumps(res["follow_up"][-1]), flush=True)
        g = torch.Generator(device="cuda").manual_seed(2817)
        e2817 = torch.randn((2817, cfg.llm.hidden_size), device="cuda", generator=g).mul_(0.02).to(torch.bfloat16)
        res["follow_up"].append(follow_up(model, e2817, lambda: e2817, a.iters, "S = 2817 drawn embeddings: (b) is the prefill alone, no tower pass"))
        print(json.dumps(res["follow_up"][-1]), flush=True)
        res["attention"] = [attention_launch(llm, r["past"], a.iters) for r in res["follow_up"]]
        print(json.dumps(res["attention"]), flush=True)
        res["chunked_prefill"] = chunked(llm, 2817, 1024, a.iters)
        print(json.dumps(res["chunked_prefill"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

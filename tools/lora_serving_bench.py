"""What serving LoRA adapters unmerged costs a batched decode step, and what it buys, one process on one GPU:

  NVILA-8B widths (seeded synthetic weights, 1 x 448^2 image + 512-token prompt per row: 769 keys), bf16, n = 2, 8 and 16 rows, ms per step of
    a. the session without the flag          (vila_llm_decode_step_batch: the code path of a build without the feature), before and after b - d,
    b. the session with the bank, every row -1    (vila_llm_decode_step_batch_lora: what the eight extra launches per layer cost when nothing is added),
    c. every row under ONE r = 64 adapter,
    d. the rows dealt over FOUR r = 64 adapters,
  b - d are the same session and graph (only row_adapter changes) and alternate inside every timing round;
  shrink and expand per call on the four stacks' shapes (rows dealt over four adapters), the bank's bytes per slot, and
  tokens/s of n requests under n DIFFERENT adapters served as the rows of one batch (prefill included), against the only way to serve them without
  the feature: one after another, each after restoring the base weights of the model and a timed merge_adapter (which drops sessions and graphs).

    python tools/lora_serving_bench.py [--steps 50] [--iters 5] [--layers 28] [--new-tokens 64] [--out profiles/lora_serving_bench.json]

Timing: a step is one hipGraph replay; a figure is the median over `--iters` timings of `--steps` back-to-back replays divided by `--steps`, after
one warm-up round; the spread is max - min of those timings.  The request comparison is wall clock around the calls, synchronised."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vila_amd import _lib, configs, lora, ops, synthetic  # noqa: E402
from vila_amd._lib import check  # noqa: E402
from vila_amd.lora_serving import AdapterBank  # noqa: E402

NS = (2, 8, 16)
R = 64


def model_and_inputs(layers, prompt_tokens, n_max):
    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = layers
    model = build_model(cfg, seed=0)
    pixels = synthetic.make_pixels(cfg, n_max, 0, device="cuda", dtype=torch.bfloat16)
    ids = torch.stack([synthetic.make_prompt(cfg, prompt_tokens, 1, i) for i in range(n_max)], 0).cuda()
    e, _, m = model._embed(ids, {"image": [pixels[i] for i in range(n_max)]})
    return cfg, model, e, m


def adapter(lcfg, seed):
    """An r = 64 adapter over the seven projections with PEFT's A and a small normal B (B = 0 would add zeros; the time does not depend on it)."""
    ad = lora.LoraAdapters(lcfg, lora.LoraConfig(r=R, alpha=16), device="cuda").init_(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for i in range(lcfg.num_hidden_layers):
            for mod in ad.cfg.target_modules:
                bt = ad.pair(i, mod)[1]
                bt.copy_((torch.randn(bt.shape, generator=g, device="cuda") * 0.01).to(torch.bfloat16))
    return ad


def time_once(graph, stream, steps):
    lib = _lib.load()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        for _ in range(steps):
            check(lib.vila_graph_launch(graph, stream.cuda_stream), "graph_launch")
        b.record(stream)
        b.synchronize()
    return a.elapsed_time(b) / steps


def stat(ts):
    return round(statistics.median(ts), 4), round((max(ts) - min(ts)) * 1e3, 1)


def plain_ms(llm, e, m, n, steps, iters):
    max_new = (iters + 1) * steps + 2
    llm._generate_batch(e[:n], m[:n], max_new, -1, None, use_graph=True)
    st = llm._bdecode
    assert st is not None and st.graph is not None and getattr(st, "lora", None) is None
    S = [int(v) for v in m[:n].sum(1).tolist()]
    ts = []
    for it in range(iters + 1):
        st.pos.copy_(torch.tensor(S, dtype=torch.int32)); st.n_out.zero_()
        t = time_once(st.graph, st.stream, steps)
        if it:
            ts.append(t)
    return stat(ts)


def bank_ms(llm, bank, e, m, n, steps, iters, names4):
    """-> {map: (ms, spread us)}: ONE session and graph, the three maps alternating inside every round."""
    S = [int(v) for v in m[:n].sum(1).tolist()]
    max_ctx = ((max(S) + 2 * steps + 255) // 256) * 256
    st = llm.batch_open(n, max_ctx, 2 * steps, adapters=bank)
    assert st.lora is not None and st.graph is not None
    llm.batch_release(st, range(st.pos.numel()))
    for b in range(n):
        llm.batch_admit(st, b, e[b, :S[b]])
    maps = {"all_minus_1": [None] * n, "one_adapter": [names4[0]] * n, "four_adapters": [names4[b % 4] for b in range(n)]}
    ts = {k: [] for k in maps}
    for it in range(iters + 1):
        for k, names in maps.items():
            for b in range(n):
                llm._set_row_adapter(st, b, names[b])
            st.pos[:n].copy_(torch.tensor(S, dtype=torch.int32)); st.n_out.zero_()
            t = time_once(st.graph, st.stream, steps)
            if it:
                ts[k].append(t)
    llm.batch_release(st, range(st.pos.numel()))
    return {k: stat(v) for k, v in ts.items()}


def op_us(fn, calls=200):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record(); b.synchronize()
    return round(a.elapsed_time(b) / calls * 1e3, 2)


def kernels_us(bank, n):
    """shrink and expand per call on layer 0 of the bank, rows dealt over slots 0..3."""
    slots = torch.tensor([b % 4 for b in range(n)], dtype=torch.int32, device="cuda")
    out = {}
    for s, K, Rs, N, cols in bank.shapes:
        x = torch.randn((n, K), device="cuda").to(torch.bfloat16)
        t = torch.zeros((n, Rs), dtype=torch.float32, device="cuda")
        d = torch.zeros((n, N), dtype=torch.float32, device="cuda")
        ends = [c0 + w for _, c0, w in cols]
        c1, c2 = (ends + [N, N])[0], (ends + [N, N])[1]
        out[s] = {"shrink_us": op_us(lambda: ops.lora_shrink(x, bank.a[s][0], bank.scale, slots, t)),
                  "expand_us": op_us(lambda: ops.lora_expand(t, bank.b[s][0], slots, d, c1, c2)), "K": K, "Rs": Rs, "N": N}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_serving_bench.json"))
    a = ap.parse_args()

    cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, max(NS))
    llm = model.llm
    S = int(m[0].sum())
    ads = [adapter(cfg.llm, 100 + i) for i in range(max(NS))]
    bank = AdapterBank(model, capacity=max(NS), r=R)
    names = [f"adapter{i}" for i in range(max(NS))]
    for nm, ad in zip(names, ads):
        bank.load(nm, ad)
    res = {"config": {"model": cfg.name, "layers": a.layers, "dtype": "bf16", "rank": R, "bank_capacity": bank.capacity,
                      "context": f"1 x 448^2 image + {a.prompt_tokens}-token prompt per row (S={S})", "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "graph replays, median of timings after one warm-up round; spread = max - min of the timings; the three maps of the "
                                "session with the bank alternate inside every round; requests: wall clock, synchronised"},
           "bank_bytes_per_slot": bank.bytes_per_slot(), "steps": [], "kernels": {}, "requests": []}
    for n in NS:
        r = {"n": n}
        r["plain_ms"], r["plain_spread_us"] = plain_ms(llm, e, m, n, a.steps, a.iters)
        for k, (ms, sp) in bank_ms(llm, bank, e, m, n, a.steps, a.iters, names).items():
            r[f"{k}_ms"], r[f"{k}_spread_us"] = ms, sp
        r["plain_again_ms"], r["plain_again_spread_us"] = plain_ms(llm, e, m, n, a.steps, a.iters)
        for k in ("all_minus_1", "one_adapter", "four_adapters"):
            r[f"{k}_minus_plain_us"] = round((r[f"{k}_ms"] - r["plain_ms"]) * 1e3, 1)
        res["steps"].append(r)
        res["kernels"][f"n{n}"] = kernels_us(bank, n)
        print(json.dumps(r), flush=True)
    print(json.dumps(res["kernels"]), flush=True)
    # n requests under n different adapters: as rows of one batch ...
    for n in NS:
        kw = dict(inputs_embeds=e[:n], attention_mask=m[:n], max_new_tokens=a.new_tokens, eos_token_id=-1, adapter=names[:n], adapters=bank)
        llm.generate(**kw)                                              # the session and its graph exist, as in a running server
        torch.cuda.synchronize(); t0 = time.perf_counter()
        llm.generate(**kw)
        torch.cuda.synchronize(); rows_s = time.perf_counter() - t0
        res["requests"].append({"n": n, "new_tokens": a.new_tokens, "rows_s": round(rows_s, 4), "rows_tokens_per_s": round(n * a.new_tokens / rows_s, 1)})
    # ... and one after another on merged weights: restore the base projections, merge, generate (merge_adapter drops sessions and graphs)
    from vila_amd.modules import _get
    keys = [f"model.layers.{i}.{lora._PARENT[mod]}.{mod}.weight" for i in range(cfg.llm.num_hidden_layers) for mod in lora.LLM_TARGETS]
    base = {k: _get(llm, k).detach().clone() for k in keys}
    per_request = []
    for i in range(max(NS)):
        n_i = int(m[i].sum())
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            for k in keys:
                _get(llm, k).copy_(base[k])
        lora.merge_adapter(model, ads[i])
        torch.cuda.synchronize(); t1 = time.perf_counter()
        llm.generate(inputs_embeds=e[i:i + 1, :n_i], max_new_tokens=a.new_tokens, eos_token_id=-1)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        per_request.append((t1 - t0, t2 - t1))
    with torch.no_grad():
        for k in keys:
            _get(llm, k).copy_(base[k])
    llm._invalidate()
    for row in res["requests"]:
        n = row["n"]
        merge_s, gen_s = sum(p[0] for p in per_request[:n]), sum(p[1] for p in per_request[:n])
        row.update(merged_restore_and_merge_s=round(merge_s, 4), merged_generate_s=round(gen_s, 4),
                   merged_tokens_per_s=round(n * a.new_tokens / (merge_s + gen_s), 1),
                   rows_over_merged=round((merge_s + gen_s) / row["rows_s"], 2))
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

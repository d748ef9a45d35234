"""What per-row sampling costs the batched decode step, one process on one GPU:

  for n in 2, 4, 8, 16 sequences of NVILA-8B widths (seeded synthetic weights, 1 x 448^2 image + 512-token prompt per row), ms per step of
    a. the greedy session                        (vila_llm_decode_step_batch: the two greedy pick launches),
    b. the sampling session, every row greedy    (vila_llm_decode_step_batch_sample: the batched sampler's three launches, rows at temperature 0),
    c. the sampling session, every row sampled   (temperature 0.2 / top_k 50 / top_p 0.9, the server's default request),
  plus the solo greedy and the solo sampled step (one sequence per weight pass: today's route for n sampled requests is n of those, one after
  another).  d_solo = solo sampled - solo greedy; the batched sampler has to stay below n x d_solo: `c_minus_a_us <= n_x_d_solo_us`.

    python tools/batch_sample_bench.py [--w4] [--steps 50] [--layers 28] [--out profiles/batch_sample_bench.json]

Timing: each step is one hipGraph replay (the graph generate() captured); a figure is the median over `--iters` timings of `--steps`
back-to-back replays, divided by `--steps`, after one warm-up round.  `--w4` measures the W4A16 steps (quantize_w4(batch_decode=True)) and
stores them under "w4" in the same file.

Per-launch times of the sampler come from a separate run under rocprofv3 of case c alone at one n (`--profile-n N`; `--layers` may be small:
the sampler's work does not depend on depth):

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/batch_sample_bench.py --profile-n 8 --layers 4
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vila_amd import _lib, configs, synthetic  # noqa: E402
from vila_amd._lib import check  # noqa: E402

NS = (2, 4, 8, 16)
SERVER_DEFAULT = (0.2, 50, 0.9)


def model_and_inputs(layers, prompt_tokens, n_max):
    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = layers
    model = build_model(cfg, seed=0)
    pixels = synthetic.make_pixels(cfg, n_max, 0, device="cuda", dtype=torch.bfloat16)
    ids = torch.stack([synthetic.make_prompt(cfg, prompt_tokens, 1, i) for i in range(n_max)], 0).cuda()
    e, _, m = model._embed(ids, {"image": [pixels[i] for i in range(n_max)]})
    return cfg, model, e, m


def time_replays(graph, stream, steps, iters):
    lib = _lib.load()
    ts = []
    with torch.cuda.stream(stream):
        for it in range(iters + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(steps):
                check(lib.vila_graph_launch(graph, stream.cuda_stream), "graph_launch")
            b.record(stream)
            b.synchronize()
            if it:                                              # the first round warms up
                ts.append(a.elapsed_time(b) / steps)
    return statistics.median(ts), (max(ts) - min(ts))


def batched_ms(llm, e, m, n, steps, iters, case):
    """case 'a': greedy session; 'b': sampling session, greedy rows; 'c': sampling session, every row at the server's default."""
    max_new = (iters + 1) * steps + 2
    sampling = None if case == "a" else [None if case == "b" else SERVER_DEFAULT + (1000 + b,) for b in range(n)]
    out = llm._generate_batch(e[:n], m[:n], max_new, -1, None, use_graph=True, sampling=sampling)       # session + captured graph
    torch.cuda.synchronize()
    st = llm._bdecode
    assert st is not None and st.graph is not None and out.shape == (n, max_new) and st.sampling == (case != "a")
    S = [int(v) for v in m[:n].sum(1).tolist()]
    st.pos.copy_(torch.tensor(S, dtype=torch.int32)); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def solo_ms(llm, e, m, steps, iters, sampled):
    max_new = (iters + 1) * steps + 2
    n = int(m[0].sum())
    kw = dict(do_sample=True, temperature=SERVER_DEFAULT[0], top_k=SERVER_DEFAULT[1], top_p=SERVER_DEFAULT[2], seed=1000) if sampled else {}
    llm.generate(inputs_embeds=e[:1, :n], max_new_tokens=max_new, eos_token_id=-1, **kw)        # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None and (st.sampling is not None) == sampled
    st.pos.fill_(n); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--w4", action="store_true", help="measure the W4A16 steps (stored under 'w4')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_sample_bench.json"))
    ap.add_argument("--profile-n", type=int, default=0, help="only replay case c at this n (for a rocprofv3 run)")
    a = ap.parse_args()

    if a.profile_n:
        cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, a.profile_n)
        if a.w4:
            model.llm.quantize_w4(keep_logical=False, batch_decode=True)
        ms, _ = batched_ms(model.llm, e, m, a.profile_n, a.steps, a.iters, "c")
        print(json.dumps({"profile_n": a.profile_n, "layers": a.layers, "sampled_batch_ms": round(ms, 4)}))
        return

    cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, max(NS))
    llm = model.llm
    if a.w4:
        llm.quantize_w4(keep_logical=False, batch_decode=True)
    S = int(m[0].sum())
    solo_g, solo_g_spread = solo_ms(llm, e, m, a.steps, a.iters, False)
    solo_s, solo_s_spread = solo_ms(llm, e, m, a.steps, a.iters, True)
    d_solo_us = (solo_s - solo_g) * 1e3
    rows = []
    for n in NS:
        r = {"n": n}
        for case, key in (("a", "greedy_session_ms"), ("b", "sampling_session_greedy_rows_ms"), ("c", "sampling_session_sampled_rows_ms")):
            ms, spread = batched_ms(llm, e, m, n, a.steps, a.iters, case)
            r[key] = round(ms, 4)
            r[key.replace("_ms", "_spread_us")] = round(spread * 1e3, 1)
        r["b_minus_a_us"] = round((r["sampling_session_greedy_rows_ms"] - r["greedy_session_ms"]) * 1e3, 1)
        r["c_minus_a_us"] = round((r["sampling_session_sampled_rows_ms"] - r["greedy_session_ms"]) * 1e3, 1)
        r["n_x_d_solo_us"] = round(n * d_solo_us, 1)
        r["within_bound"] = bool(r["c_minus_a_us"] <= r["n_x_d_solo_us"])
        r["sampled_batch_tok_s"] = round(n * 1e3 / r["sampling_session_sampled_rows_ms"], 1)
        r["solo_sampled_tok_s"] = round(1e3 / solo_s, 1)            # n sampled sequences one after another: the aggregate is the solo rate
        r["greedy_batch_tok_s"] = round(n * 1e3 / r["greedy_session_ms"], 1)
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "context": f"1 x 448^2 image + {a.prompt_tokens}-token prompt per row (S={S})",
                      "steps_per_timing": a.steps, "timings": a.iters, "method": "graph replays, median of timings after one warm-up round",
                      "sampling": "temperature 0.2, top_k 50, top_p 0.9"},
           "solo": {"greedy_ms": round(solo_g, 4), "sampled_ms": round(solo_s, 4), "d_solo_us": round(d_solo_us, 1),
                    "greedy_spread_us": round(solo_g_spread * 1e3, 1), "sampled_spread_us": round(solo_s_spread * 1e3, 1)},
           "rows": rows}
    print(json.dumps(res["solo"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    old["w4" if a.w4 else "bf16"] = res
    with open(a.out, "w") as f:
        json.dump(old, f, indent=1)


if __name__ == "__main__":
    main()

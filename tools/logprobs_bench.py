"""What per-token logprobs cost a decode step, one process on one GPU:

  NVILA-8B widths (seeded synthetic weights, 1 x 448^2 image + 512-token prompt per row: 769 keys), bf16 and W4A16, ms per step of
    solo greedy, solo sampled (temperature 0.2 / top_k 50 / top_p 0.9), and the greedy batched step at n = 2, 8 and 16 rows, each
      a. without the flag     (the plain session: the code path of a build without the feature),
      b. with logprobs=True   (the same step, and behind it in the same graph the two launches of vila_logprobs_f32: all 20 alternatives, n x 608 KB read).

    python tools/logprobs_bench.py [--steps 50] [--iters 5] [--rounds 2] [--layers 28] [--out profiles/logprobs_bench.json]

Timing: each step is one hipGraph replay (the graph generate() captured); a timing is `--steps` back-to-back replays between two device events,
divided by `--steps`.  The two sessions of a configuration alternate `--rounds` times (a, b, a, b: each round opens its session and captures its
graph anew) with `--iters` timings each after one warm-up timing; a figure is the median over a case's rounds x iters timings, the spread is
max - min of them.  The baseline of every delta is case a of the same run."""
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

NS = (2, 8, 16)
SERVER_DEFAULT = (0.2, 50, 0.9)
CASES = (("none", None), ("logprobs", 20))


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
    return ts


def solo_ts(llm, e, m, steps, iters, sampled, k):
    max_new = (iters + 1) * steps + 2
    n = int(m[0].sum())
    sampling = SERVER_DEFAULT + (1000,) if sampled else None
    kw = {} if k is None else dict(logprobs=k)
    llm._generate_solo(e[:1, :n], None, max_new, -1, sampling, True, False, None, None, None, **kw)      # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None and (st.sampling is not None) == sampled and (st.lp is not None) == (k is not None)
    st.pos.fill_(n); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def batched_ts(llm, e, m, n, steps, iters, k):
    max_new = (iters + 1) * steps + 2
    kw = {} if k is None else dict(logprobs=k)
    out = llm._generate_batch(e[:n], m[:n], max_new, -1, None, use_graph=True, **kw)                     # session + captured graph
    torch.cuda.synchronize()
    st = llm._bdecode
    ids = out if k is None else out[0]
    assert st is not None and st.graph is not None and ids.shape == (n, max_new) and (st.lp is not None) == (k is not None)
    S = [int(v) for v in m[:n].sum(1).tolist()]
    st.pos.copy_(torch.tensor(S, dtype=torch.int32)); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs_bench.json"))
    a = ap.parse_args()

    cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, max(NS))
    llm = model.llm
    S = int(m[0].sum())
    configs_ = [("solo_greedy", lambda k: solo_ts(llm, e, m, a.steps, a.iters, False, k)),
                ("solo_sampled", lambda k: solo_ts(llm, e, m, a.steps, a.iters, True, k))]
    configs_ += [(f"batch_{n}", (lambda k, n=n: batched_ts(llm, e, m, n, a.steps, a.iters, k))) for n in NS]
    rows = []
    for dtype in ("bf16", "w4"):
        if dtype == "w4":
            llm.quantize_w4(batch_decode=True)
        for name, run in configs_:
            ts = {case: [] for case, _ in CASES}
            for _ in range(a.rounds):                           # a, b, a, b: the two sessions alternate within the run
                for case, k in CASES:
                    ts[case] += run(k)
            r = {"dtype": dtype, "config": name}
            for case, _ in CASES:
                r[f"{case}_ms"] = round(statistics.median(ts[case]), 4)
                r[f"{case}_spread_us"] = round((max(ts[case]) - min(ts[case])) * 1e3, 1)
            r["logprobs_minus_none_us"] = round((r["logprobs_ms"] - r["none_ms"]) * 1e3, 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "dtypes": ["bf16", "w4 (quantize_w4(batch_decode=True))"], "vocab": cfg.llm.vocab_size,
                      "context": f"1 x 448^2 image + {a.prompt_tokens}-token prompt per row (S={S})", "steps_per_timing": a.steps,
                      "timings_per_case": a.rounds * a.iters,
                      "method": "graph replays between device events; the plain and the flagged session alternate within the run; median of a case's "
                                "timings after one warm-up timing per session; spread = max - min of the case's timings",
                      "solo_sampled": "temperature 0.2, top_k 50, top_p 0.9", "baseline": "none_ms of the same run (the session without the flag)",
                      "yardstick": "the batched sampler's three launches cost 50 - 72 us per step (profiles/batch_sample_bench.json)"},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

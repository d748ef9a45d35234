"""Greedy speculative decoding, measured in one process on one GPU: the verify step (vila_llm_decode_step_verify, attn_decode.hip
bdec_attn_shared_kernel) at NVILA-8B widths with seeded synthetic weights.

  for bf16 and W4, 769 and 8192 cached keys, n = 4 / 8 / 16 rows per step:
    * ms per verify step (one hipGraph replay: draft + forward of n rows + accept),
    * the solo step at that context and the existing batched step at equal n and keys (n rows in n slots), both untouched code,
    * break-even acceptance t_verify / t_solo - 1: accepted drafts per step from which speculation pays,
    * tokens/s in candidate mode at 0 % acceptance (a candidate that is wrong everywhere: 1 token per step) and at 100 % (the candidate is the
      model's own output, recorded by a run that drafts nothing: n tokens per step).  These are the two ends; synthetic weights have no meaningful
      acceptance rate of their own.

    python tools/spec_decode_bench.py [--steps 10] [--iters 3] [--layers 28] [--out profiles/spec_decode_bench.json]

Timing: HIP events around `--steps` back-to-back replays, warm (one untimed round first), median of `--iters` rounds, divided by `--steps`.  The KV
caches are filled with seeded noise instead of a prefill (a step's time does not depend on the values); the solo step decodes behind a real prefill.
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

from vila_amd import _lib, configs  # noqa: E402
from vila_amd._lib import check  # noqa: E402
from vila_amd.modules import _capture  # noqa: E402

NS = (4, 8, 16)
KEYS = (769, 8192)


def replay(graph, stream, steps):
    """ms for `steps` back-to-back replays"""
    lib = _lib.load()
    with torch.cuda.stream(stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(steps):
            check(lib.vila_graph_launch(graph, stream.cuda_stream), "graph_launch")
        b.record(stream)
        b.synchronize()
    return a.elapsed_time(b)


def noise(cache, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for t in (cache.k, cache.v):
        for layer in range(t.shape[0]):
            t[layer].copy_(torch.randn(t.shape[1:], device="cuda", generator=g, dtype=torch.float32).mul_(0.5))


def batched_ms(llm, n, keys, steps, iters):
    room = (iters + 1) * steps + 2
    llm._drop_batch_session()
    st = llm.batch_open(n, ((keys + room + 255) // 256) * 256, room)
    noise(st.cache, keys + n)
    ts = []
    for it in range(iters + 1):
        st.pos.fill_(keys); st.n_out.zero_(); st.token.fill_(17)
        torch.cuda.synchronize()
        ts.append(replay(st.graph, st.stream, steps) / steps)
    llm._drop_batch_session()
    return statistics.median(ts[1:])


def solo_ms(llm, keys, steps, iters):
    room = steps + 2
    g = torch.Generator(device="cuda").manual_seed(keys)
    e = torch.randn((1, keys, llm.lcfg.hidden_size), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16)
    llm.generate(inputs_embeds=e, max_new_tokens=room, eos_token_id=-1)                       # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None
    ts = []
    for it in range(iters + 1):
        st.pos.fill_(keys); st.n_out.zero_()
        torch.cuda.synchronize()
        ts.append(replay(st.graph, st.stream, steps) / steps)
    llm._drop_decode_session()
    return statistics.median(ts[1:])


def verify_ms(llm, n, keys, steps, iters):
    """-> (ms per step at 0 % acceptance, at 100 %, tokens per step seen at 0 %, at 100 %)"""
    room = n * steps + n
    cache = llm.new_cache(((keys + room + 255) // 256) * 256)
    noise(cache, keys + n)
    llm._drop_session("_vdecode")
    st = llm._verify_session(cache, n, room, 2)

    def reset(n_cand):
        st.pos.fill_(keys); st.n_out.zero_(); st.n_hist.fill_(1); st.token.fill_(17); st.n_cand.fill_(n_cand)
    reset(0)
    _capture(st, lambda: llm.verify_step(cache, st), lambda: reset(0))
    # the model's own output from this state: n * steps replays that draft nothing
    reset(0)
    torch.cuda.synchronize()
    replay(st.graph, st.stream, n * steps)
    own = st.out_ids[:n * steps].clone()
    out = []
    for cand, n_cand in ((own + 1, n * steps), (own, n * steps)):     # wrong everywhere / right everywhere
        st.cand[:n * steps].copy_(cand)
        ts = []
        for it in range(iters + 1):
            reset(n_cand)
            torch.cuda.synchronize()
            ts.append(replay(st.graph, st.stream, steps) / steps)
        out.append((statistics.median(ts[1:]), int(st.n_out.item()) / steps))
    assert torch.equal(st.out_ids[:n * steps], own), "speculation changed the ids"
    llm._drop_session("_vdecode")
    return out[0][0], out[1][0], out[0][1], out[1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_decode_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = a.layers
    llm = build_model(cfg, seed=0).llm
    rows = []
    for dtype in ("bf16", "w4"):
        if dtype == "w4":
            llm.quantize_w4(keep_logical=False, batch_decode=True)
        for keys in KEYS:
            solo = solo_ms(llm, keys, a.steps, a.iters)
            for n in NS:
                bat = batched_ms(llm, n, keys, a.steps, a.iters)
                v0, v100, t0, t100 = verify_ms(llm, n, keys, a.steps, a.iters)
                r = {"dtype": dtype, "keys": keys, "n": n, "solo_ms": round(solo, 4), "batched_ms": round(bat, 4), "verify_ms": round(v0, 4),
                     "verify_ms_all_accepted": round(v100, 4), "verify_over_batched": round(v0 / bat, 3), "break_even_accepted_per_step": round(v0 / solo - 1, 3),
                     "solo_tok_s": round(1e3 / solo, 1), "tok_s_0pct": round(t0 * 1e3 / v0, 1), "tok_s_100pct": round(t100 * 1e3 / v100, 1),
                     "tokens_per_step_0pct": t0, "tokens_per_step_100pct": t100}
                rows.append(r)
                print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "HIP events around back-to-back graph replays, warm, median",
                      "break_even_accepted_per_step": "verify_ms / solo_ms - 1", "verify_over_batched": "verify_ms / batched_ms at equal n and keys"},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Batched decode past 2048 cached positions, measured in one process on one GPU: the walking attention of the batched step
(attn_decode.hip bdec_attn_walk_kernel) at NVILA-8B widths with seeded synthetic weights.

  for bf16 and W4, contexts of about 2400 (dynamic_s2's 2304 image tokens + a prompt) and 8192 keys, n = 2 / 8 / 16 rows:
    * ms per batched step and aggregate tokens/s for each slice cap (8 / 16 / 32: vila_decode_batch_force_slices; NSL = min(cap, chunks of
      the capacity), so at 2400 keys caps 16 and 32 launch the same grid),
    * what the rows cost without the feature: n x the solo step at that context (rows served one after another),
    * the existing batched step at the same n in a 2048-position session (1792 keys per row).

    python tools/long_batch_decode_bench.py [--steps 20] [--iters 3] [--layers 28] [--out profiles/long_batch_decode_bench.json]

Timing: a step is one hipGraph replay; a figure is the median over `--iters` timings of `--steps` back-to-back replays (one more warms up),
divided by `--steps`.  Positions advance during the timed replays (<= (iters + 1) * steps keys).  The batched rows' KV caches are filled with
seeded noise instead of a prefill (the step's time does not depend on the values; the prefill of 16 x 8192 tokens would only cost time); the solo
step decodes behind a real prefill of random embeddings.
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

NS = (2, 8, 16)
CTXS = (2400, 8192)
CAPS = (8, 16, 32)
SHORT_KEYS = 1792


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
            if it:
                ts.append(a.elapsed_time(b) / steps)
    return statistics.median(ts)


def batched_ms(llm, n, keys, cap, steps, iters):
    """ms per batched step of n rows with `keys` cached positions each; cap = slices forced for the walking form (0 = automatic)."""
    lib = _lib.load()
    room = (iters + 1) * steps + 2
    max_ctx = ((keys + room + 255) // 256) * 256
    llm._drop_batch_session()                                   # the captured graph bakes the slice count
    lib.vila_decode_batch_force_slices(int(cap))
    try:
        st = llm.batch_open(n, max_ctx, room)
    finally:
        lib.vila_decode_batch_force_slices(0)
    g = torch.Generator(device="cuda").manual_seed(keys + n)
    for t in (st.cache.k, st.cache.v):
        for layer in range(t.shape[0]):                         # (layer by layer: no fp32 copy of the whole cache)
            t[layer].copy_(torch.randn(t.shape[1:], device="cuda", generator=g, dtype=torch.float32).mul_(0.5))
    st.pos.fill_(keys); st.n_out.zero_(); st.token.fill_(17)
    torch.cuda.synchronize()
    ms = time_replays(st.graph, st.stream, steps, iters)
    slices = st.attn_slices
    llm._drop_batch_session()
    return ms, slices, max_ctx


def solo_ms(llm, keys, steps, iters):
    room = (iters + 1) * steps + 2
    g = torch.Generator(device="cuda").manual_seed(keys)
    e = torch.randn((1, keys, llm.lcfg.hidden_size), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16)
    llm.generate(inputs_embeds=e, max_new_tokens=room, eos_token_id=-1)                       # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None
    st.pos.fill_(keys); st.n_out.zero_()
    ms = time_replays(st.graph, st.stream, steps, iters)
    llm._drop_decode_session()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_batch_decode_bench.json"))
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
        short = {n: batched_ms(llm, n, SHORT_KEYS, 0, a.steps, a.iters)[0] for n in NS}
        for keys in CTXS:
            solo = solo_ms(llm, keys, a.steps, a.iters)
            for n in NS:
                r = {"dtype": dtype, "keys": keys, "n": n, "solo_ms": round(solo, 4), "solo_serial_tok_s": round(1e3 / solo, 1),
                     "short_batch_ms": round(short[n], 4), "short_batch_keys": SHORT_KEYS}
                for cap in CAPS:
                    ms, slices, max_ctx = batched_ms(llm, n, keys, cap, a.steps, a.iters)
                    r["max_ctx"] = max_ctx
                    r[f"cap{cap}"] = {"slices": slices, "ms": round(ms, 4), "tok_s": round(n * 1e3 / ms, 1),
                                      "over_solo_serial": round(n * solo / ms, 2), "over_short_batch": round(ms / short[n], 3)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "steps_per_timing": a.steps, "timings": a.iters, "method": "graph replays",
                      "over_solo_serial": "n x solo_ms / batched ms (speed-up over serving the rows one after another)",
                      "over_short_batch": "batched ms / ms of the <= 2048-position batched step at the same n"},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

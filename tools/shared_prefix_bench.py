"""Batched decode over a shared prompt prefix, measured in one process on one GPU: the step of a prefix session (vila_llm_decode_step_batch_prefix,
attn_decode.hip bdec_attn_shared_kernel<.., true> + bdec_attn_walk_kernel<.., true> + bdec_attn_prefix_merge_kernel) at NVILA-8B widths with seeded
synthetic weights, against the ordinary session that holds n full copies of the same keys (untouched code).

  for bf16 and W4, shared lengths 256 / 2304 / 8192 plus a 48-token private tail, n = 2 / 8 / 16 rows:
    * ms per step of the prefix session (every row shares) and of the ordinary session at the same positions, and their ratio,
    * K/V bytes held by either session for these rows (57,344 B per position and row at NVILA-8B shapes),
  and per shared length (bf16 and W4 prefill as the model is configured):
    * ms to admit a sharer (batch_admit(share=True): prefill of the 48-token tail onto the prefix, copy of the tail's K/V) against an ordinary
      admission of the same prompt (prefill of S + 48 tokens).

    python tools/shared_prefix_bench.py [--steps 20] [--iters 7] [--layers 28] [--out profiles/shared_prefix_bench.json]

Timing of a step: HIP events around `--steps` back-to-back graph replays, warm (one untimed round first), median of `--iters` rounds, divided by
`--steps`; the two sessions are alive at once and their rounds alternate.  The KV caches are filled with seeded noise instead of a prefill (a
step's time does not depend on the values).  Timing of an admission: wall clock around the call between device synchronisations (an admission ends
with the host reading the first token), warm, median.
"""
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

from vila_amd import _lib, configs  # noqa: E402
from vila_amd._lib import check  # noqa: E402

NS = (2, 8, 16)
SHARED = (256, 2304, 8192)
TAIL = 48


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


def step_ms(llm, n, S, steps, iters):
    """-> (ms per step of the ordinary session, of the prefix session).  Both sessions are alive at once and their timing rounds alternate."""
    room = (iters + 1) * steps + 2
    keys = S + TAIL
    arms = []
    for shared in (False, True):
        llm._drop_batch_session()
        st = llm.batch_open(n, ((keys + room + 255) // 256) * 256, room, shared_prefix=shared)
        llm._bdecode = None                              # keep this session alive beside the next one; dropped by hand below
        noise(st.cache, keys + n)
        if shared:
            st.shared_len.fill_(S); st.uses.fill_(1)
        arms.append((st, []))
    for it in range(iters + 1):
        for st, ts in arms:                              # the arms alternate inside every round
            st.pos.fill_(keys); st.n_out.zero_(); st.token.fill_(17)
            torch.cuda.synchronize()
            ts.append(replay(st.graph, st.stream, steps) / steps)
    for st, _ in arms:
        llm._bdecode = st
        llm._drop_batch_session()
    return tuple(statistics.median(ts[1:]) for _, ts in arms)


def admit_ms(llm, S, iters):
    """-> (ms to admit a sharer of a pinned prefix of S positions with a 48-token tail, ms to admit the same prompt as an ordinary row)"""
    P, H = S + TAIL, llm.lcfg.hidden_size
    g = torch.Generator(device="cuda").manual_seed(S)
    e = torch.randn((P, H), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16)
    tails = [torch.randn((TAIL, H), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16) for _ in range(2)]
    llm._drop_batch_session()
    st = llm.batch_open(2, ((P + 8 + 255) // 256) * 256, 8, shared_prefix=True)
    assert llm.batch_set_prefix(st, e, prefix_len=S) == S
    share, plain = [], []
    for it in range(iters + 1):
        for ts, call in ((share, lambda: llm.batch_admit(st, 1, tails[it % 2], share=True, first_row=S)), (plain, lambda: llm.batch_admit(st, 0, e))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            llm.batch_release(st, [0, 1])
    llm._drop_batch_session()
    return statistics.median(share[1:]), statistics.median(plain[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = a.layers
    llm = build_model(cfg, seed=0).llm
    c = llm.lcfg
    kv_row = c.num_hidden_layers * 2 * c.num_key_value_heads * c.head_dim * 2          # K and V bytes per position and row
    rows, admits = [], []
    for dtype in ("bf16", "w4"):
        if dtype == "w4":
            llm.quantize_w4(keep_logical=False, batch_decode=True)
        for S in SHARED:
            sh, pl = admit_ms(llm, S, a.iters)
            r = {"dtype": dtype, "shared_len": S, "tail": TAIL, "admit_sharer_ms": round(sh, 3), "admit_ordinary_ms": round(pl, 3),
                 "ordinary_over_sharer": round(pl / sh, 2)}
            admits.append(r)
            print(json.dumps(r), flush=True)
            for n in NS:
                plain, shared = step_ms(llm, n, S, a.steps, a.iters)
                r = {"dtype": dtype, "shared_len": S, "tail": TAIL, "n": n, "ordinary_ms": round(plain, 4), "prefix_ms": round(shared, 4),
                     "prefix_over_ordinary": round(shared / plain, 3), "kv_bytes_ordinary": n * (S + TAIL) * kv_row,
                     "kv_bytes_prefix": (S + n * TAIL) * kv_row}
                rows.append(r)
                print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "steps: HIP events around back-to-back graph replays, warm, median, the two sessions' rounds alternating; admissions: wall clock between device synchronisations, warm, median",
                      "ordinary_ms": "the batched step of a session whose n rows each hold shared_len + tail keys of their own (the code the parent commit runs)",
                      "prefix_ms": "the step of batch_open(shared_prefix=True) with every row sharing shared_len keys and holding tail keys of its own",
                      "kv_bytes": "K and V bytes the rows' keys occupy, all layers; the prefix session counts the shared keys once"},
           "admissions": admits, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

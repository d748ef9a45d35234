"""W4A16 prefill measurements, one process on one GPU:

  1. TF/s of vila_gemm_w4_bf16 (int4 weights) against the bf16 GEMM (vila_gemm_bf16_ws) on the NVILA-8B qkv / o / gate-up / down shapes
     at M = 769 and M = 64;
  2. the LLM prefill (all 28 layers, generation form: last-row logits, KV cache filled) of NVILA-8B widths, bf16 vs W4, at S = 769 and 64;
  3. torch.cuda.memory_allocated before and after release_bf16 (quantize_w4(prefill=True) then release_bf16_projections()).

    python tools/w4_prefill_bench.py [--iters 20] [--layers 28] [--out profiles/w4_prefill_bench.json]

Timing: every measured call is captured in a hipGraph (torch.cuda.graph) and replayed, so the host's launch path (Python, ctypes, workspace
allocation) is not in the numbers; a GEMM row is the median over `--iters` replays of a graph of `REPS` back-to-back launches, divided by REPS.
Cache state is reported per row: "warm" = back to back, so weights that fit the 256 MB MALL (every int4 matrix here, 9-72 MB; of the bf16 ones
all but gate/up, 272 MB) are served from it after the first launch; "cold" = a 1 GiB buffer is overwritten before every launch inside the
graph and that flush's own time (measured alone the same way) is subtracted.  The prefill rows replay one whole prefill per graph (warm).
If a capture fails the row falls back to eager launches between events and says so ("method").
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vila_amd import configs, ops, synthetic  # noqa: E402
from vila_amd.quant import W4Matrix, rope_interleave_rows  # noqa: E402


REPS = 10


def _median_replay(g, iters):
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def graph_time(fn, iters, reps=REPS):
    """-> (us per call, method): median replay time of a graph holding `reps` calls of fn, divided by reps."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        return _median_replay(g, iters) / reps, "graph"
    except Exception as e:                     # noqa: BLE001  (a launch path that cannot be captured: time it eagerly, and say so)
        print(f"graph capture failed ({type(e).__name__}: {e}); eager timing", flush=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / reps)
        ts.sort()
        return ts[len(ts) // 2], "eager"


_flush_buf = None


def _flush():
    global _flush_buf
    if _flush_buf is None:
        _flush_buf = torch.empty(1 << 30, device="cuda", dtype=torch.uint8)
    _flush_buf.fill_(1)


def cold_time(fn, iters):
    t, m = graph_time(lambda: (_flush(), fn()), iters)
    f, _ = graph_time(_flush, iters)
    return t - f, m


def gemm_rows(iters):
    c = configs.nvila_8b().llm
    H, F, hd, nq, nkv = c.hidden_size, c.intermediate_size, c.head_dim, c.num_attention_heads, c.num_key_value_heads
    QKV = (nq + 2 * nkv) * hd
    shapes = [("qkv", QKV, H), ("o_proj", H, H), ("gate_up", F, H), ("down", H, F)]
    rows = []
    g = torch.Generator().manual_seed(0)
    for name, N, K in shapes:
        if name == "gate_up":
            wg, wu = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda(), (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
            mat = W4Matrix.pack(wg, wu, keep_logical=False)
        elif name == "qkv":
            wg = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
            wu = None
            mat = W4Matrix.pack(wg, row_perm=rope_interleave_rows(nq + nkv, nq + 2 * nkv, hd, device="cuda"), keep_logical=False)
        else:
            wg = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
            wu = None
            mat = W4Matrix.pack(wg, keep_logical=False)
        bias = torch.zeros(N, device="cuda", dtype=torch.bfloat16) if name == "qkv" else None
        n_out = 2 * N if name == "gate_up" else N
        for M in (769, 64):
            x = (torch.randn(M, K, generator=g)).to(torch.bfloat16).cuda()
            out4 = torch.empty((M, N), device="cuda", dtype=torch.bfloat16)
            heads = (nq, nkv, hd) if name == "qkv" else None
            ws = torch.empty((8 * M * max(N, H) * 4 + (1 << 20),), device="cuda", dtype=torch.uint8)
            outb = torch.empty((M, N), device="cuda", dtype=torch.bfloat16)
            f4 = lambda: ops.gemm_w4(x, mat, bias=bias, out=out4, heads=heads)                                    # noqa: E731
            if name == "gate_up":
                fb = lambda: ops.gemm(x, wg, epi=ops.EPI_GATEUP, w2=wu, out=outb, ws=ws)                           # noqa: E731
            else:
                fb = lambda: ops.gemm(x, wg, bias=bias, out=outb, ws=ws)                                           # noqa: E731
            flop = 2.0 * M * n_out * K
            for cache, timer in (("warm", graph_time), ("cold", cold_time)):
                t4, m4 = timer(f4, iters)
                tb, mb = timer(fb, iters)
                rows.append({"shape": name, "M": M, "N": n_out, "K": K, "cache": cache, "w4_us": round(t4, 2), "bf16_us": round(tb, 2),
                             "w4_tflops": round(flop / t4 / 1e6, 1), "bf16_tflops": round(flop / tb / 1e6, 1),
                             "w4_weight_bytes": mat.nbytes(), "bf16_weight_bytes": n_out * K * 2, "method": f"{m4}/{mb}"})
                print(json.dumps(rows[-1]), flush=True)
        del mat, wg, wu
        torch.cuda.empty_cache()
    return rows


def prefill_rows(iters, layers):
    from vila_amd.vlm import build_model
    cfg = configs.reduced_8b(layers_v=1, layers_l=layers, vocab=152064)
    model = build_model(cfg, seed=0)
    llm = model.llm
    out = {"layers": layers}

    def run(S):
        e = (torch.randn(S, cfg.llm.hidden_size, generator=torch.Generator().manual_seed(S)) * 0.02).to(torch.bfloat16).cuda()
        pos = torch.arange(S, dtype=torch.int32, device="cuda")
        last = torch.full((1,), S - 1, dtype=torch.int32, device="cuda")
        cache = llm.new_cache(((S + 255) // 256) * 256)
        t, m = graph_time(lambda: llm.prefill_packed(e, pos, None, S, cache=cache, last_rows=last), iters, reps=1)
        out["method"] = m
        return t

    for S in (769, 64):
        out[f"bf16_S{S}_us"] = round(run(S), 1)
    llm.quantize_w4(keep_logical=False, prefill=True)
    for S in (769, 64):
        out[f"w4_S{S}_us"] = round(run(S), 1)
        out[f"w4_over_bf16_S{S}"] = round(out[f"w4_S{S}_us"] / out[f"bf16_S{S}_us"], 3)
    print(json.dumps(out), flush=True)
    torch.cuda.synchronize()
    proj = sum(p.numel() * p.element_size() for n, p in llm.named_parameters() if n.endswith("_proj.weight"))
    m0 = torch.cuda.memory_allocated()
    freed = llm.release_bf16_projections()
    torch.cuda.synchronize()
    m1 = torch.cuda.memory_allocated()
    mem = {"memory_allocated_before": m0, "memory_allocated_after": m1, "drop": m0 - m1, "bf16_projection_bytes": proj,
           "released_bytes": freed, "int4_projection_bytes": llm._w4.nbytes()}
    for S in (769, 64):
        mem[f"w4_released_S{S}_us"] = round(run(S), 1)
    print(json.dumps(mem), flush=True)
    return out, mem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "gemm": gemm_rows(a.iters)}
    res["prefill"], res["memory"] = prefill_rows(a.iters, a.layers)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

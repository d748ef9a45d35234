"""What a LoRA step costs next to the full SFT step, one process on one GPU, NVILA-8B shapes with seeded synthetic weights, a micro-batch of
4 samples x (1 x 448^2 image + 512 text tokens) = 4 x 769 packed positions, r = 64, alpha = 16, the projector tuned:

  a. the LoRA step (vila_amd/lora.py LoRATrainer.step) against the full SFT step (train.SFTTrainer.step, unchanged) of the SAME run;
  b. the LoRA step against the same trainer with ZERO target modules (frozen-LLM forward + dgrad only): the adapters' own cost;
  c. each of the three kernels (vila_amd/csrc/lora.hip) alone at every shape the step uses, next to bytes moved / 8 TB/s;
  d. torch.cuda.max_memory_allocated of the trainers.

    python tools/lora_bench.py [--rounds 5] [--steps 3] [--layers 28] [--out profiles/lora_bench.json]

Timing.  Steps: the sessions ALTERNATE inside the run (round i times `--steps` steps of every session, one after another, after one warm-up round);
a figure is the median over the rounds of (host clock around the steps, ending in a device synchronise) / steps, the spread is max - min over the
rounds.  Kernels: device events around `--kernel-reps` back-to-back calls of the C entry point with a preallocated workspace, median over five
such timings after a warm-up.  "bytes" are the operand and result bytes the algorithm has to move once (re-reads from L2 not counted)."""
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

from vila_amd import configs, synthetic  # noqa: E402

HBM_TBS = 8.0


def kernel_shapes(c, T, r):
    """Every (kernel, shape, uses per layer, where) of one LoRA step at hidden H, intermediate I, q / kv widths, T packed rows."""
    H, I, q, kv = c.hidden_size, c.intermediate_size, c.q_size, c.kv_size
    down = [((T, H, 3 * r), 1, "t of q|k|v"), ((T, q, r), 1, "t of o"), ((T, H, 2 * r), 1, "t of gate|up"), ((T, I, r), 1, "t of down"),
            ((T, H, r), 1, "dt of down"), ((T, I, r), 2, "dt of gate, up"), ((T, H, r), 1, "dt of o"), ((T, q, r), 1, "dt of q"), ((T, kv, r), 2, "dt of k, v")]
    up = [((T, q, r, False), 1, "u of q"), ((T, kv, r, False), 2, "u of k, v"), ((T, H, r, True), 2, "u of o, down (+ residual)"),
          ((T, I, r, False), 2, "u of gate, up"), ((T, I, r, False), 1, "dx of down"), ((T, H, 2 * r, False), 1, "dx of gate|up"),
          ((T, q, r, False), 1, "dx of o"), ((T, H, 3 * r, False), 1, "dx of q|k|v")]
    wgrad = [((T, r, H), 2, "dBt of down, o"), ((T, r, q), 1, "dBt of q"), ((T, r, I), 2, "dBt of gate, up"), ((T, r, kv), 2, "dBt of k, v"),
             ((T, r, I), 1, "dA of down"), ((T, 2 * r, H), 1, "dA of gate|up"), ((T, r, q), 1, "dA of o"), ((T, 3 * r, H), 1, "dA of q|k|v")]
    return down, up, wgrad


def kernel_bytes(kind, shape):
    if kind == "down":
        M, K, R = shape
        return 2 * (M * K + R * K + M * R)
    if kind == "up":
        M, N, R, res = shape
        return 2 * (M * N * (2 if res else 1) + M * R + R * N)
    M, R, C = shape
    return 2 * (M * C + M * R + R * C)


def time_kernel(call, reps):
    ts = []
    for it in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        if it:
            ts.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(ts), max(ts) - min(ts)


def bench_kernels(c, T, r, reps):
    from vila_amd import _lib
    from vila_amd._lib import check
    from vila_amd.ops import _stream
    lib = _lib.load()
    rnd = lambda *s: (torch.randn(*s, device="cuda") * 0.5).to(torch.bfloat16)
    rows, seen = [], set()
    down, up, wgrad = kernel_shapes(c, T, r)
    for kind, cases in (("down", down), ("up", up), ("wgrad", wgrad)):
        for shape, uses, where in cases:
            if (kind, shape) in seen:
                prev = next(x for x in rows if x["kernel"] == kind and tuple(x["shape"]) == tuple(int(v) for v in shape))
                prev["uses_per_layer"] += uses
                prev["where"] += "; " + where
                continue
            seen.add((kind, shape))
            if kind == "down":
                M, K, R = shape
                x, a, o = rnd(M, K), rnd(R, K), torch.empty((M, R), device="cuda", dtype=torch.bfloat16)
                n = int(lib.vila_lora_down_workspace_bytes(M, K, R))
                ws = torch.empty((max(n, 16),), device="cuda", dtype=torch.uint8)
                call = lambda: check(lib.vila_lora_down_bf16(x.data_ptr(), K, a.data_ptr(), K, o.data_ptr(), R, M, K, R, 0.25, ws.data_ptr(), n, _stream()), "lora_down")
            elif kind == "up":
                M, N, R, res = shape
                t, bt, o = rnd(M, R), rnd(R, N), torch.empty((M, N), device="cuda", dtype=torch.bfloat16)
                rs = rnd(M, N) if res else None
                call = lambda: check(lib.vila_lora_up_bf16(t.data_ptr(), R, bt.data_ptr(), N, None if rs is None else rs.data_ptr(), N, o.data_ptr(), N, M, N, R,
                                                           0.25, None, 0, _stream()), "lora_up")
            else:
                M, R, C = shape
                l, x, o = rnd(M, R), rnd(M, C), torch.empty((R, C), device="cuda", dtype=torch.bfloat16)
                n = int(lib.vila_lora_wgrad_workspace_bytes(M, R, C))
                ws = torch.empty((max(n, 16),), device="cuda", dtype=torch.uint8)
                call = lambda: check(lib.vila_lora_wgrad_bf16(l.data_ptr(), R, x.data_ptr(), C, o.data_ptr(), C, M, R, C, 0.25, 0, ws.data_ptr(), n, _stream()), "lora_wgrad")
            call()
            torch.cuda.synchronize()
            us, spread = time_kernel(call, reps)
            nbytes = kernel_bytes(kind, shape)
            rows.append({"kernel": kind, "shape": [int(v) for v in shape], "uses_per_layer": uses, "where": where, "us": round(us, 2), "spread_us": round(spread, 2),
                         "bytes": nbytes, "us_at_8TBs": round(nbytes / (HBM_TBS * 1e6), 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--micro-batch", type=int, default=4)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--no-full", action="store_true", help="skip the full SFT trainer (113 GB of optimizer state)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench measures on the GPU; there is none here")
    from vila_amd.lora import LoraConfig, LoRATrainer
    from vila_amd.train import SFTTrainer
    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = a.layers
    b = a.micro_batch
    pixels = synthetic.make_pixels(cfg, b, 0, device="cuda", dtype=torch.bfloat16)
    ids = torch.stack([synthetic.make_prompt(cfg, a.prompt_tokens, 1, i) for i in range(b)], 0)
    labels = ids.clone()
    labels[:, : 1 + a.prompt_tokens - 256] = -100
    images = [pixels[i] for i in range(b)]
    T = b * (cfg.tokens_per_tile + 1 + a.prompt_tokens)

    sessions, memory = {}, {}

    def add(name, make):
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tr = make()
        loss = float(tr.step(ids, images, labels))          # warm-up: every shape of the timed window
        torch.cuda.synchronize()
        memory[name] = {"max_memory_allocated": int(torch.cuda.max_memory_allocated() - resident), "resident_before": int(resident),
                        "state_numel": int(tr.flat.numel)}
        sessions[name] = (tr, loss)

    add("lora", lambda: LoRATrainer(build_model(cfg, seed=0), LoraConfig(r=a.rank, alpha=16), tune_mm_projector=True, lr=2e-4))
    add("lora_zero_targets", lambda: LoRATrainer(build_model(cfg, seed=0), LoraConfig(r=a.rank, alpha=16, target_modules=()), tune_mm_projector=True, lr=2e-4))
    if not a.no_full:
        add("full_sft", lambda: SFTTrainer(build_model(cfg, seed=0), lr=2e-5, weight_decay=0.0))

    times = {n: [] for n in sessions}
    losses = {n: l for n, (_, l) in sessions.items()}
    for rnd in range(a.rounds + 1):
        for name, (tr, _) in sessions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = tr.step(ids, images, labels)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps * 1e3
            if rnd:
                times[name].append(dt)
            losses[name] = float(loss)
    steps = {n: {"ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "rounds_ms": [round(x, 3) for x in v], "last_loss": losses[n]}
             for n, v in times.items()}
    out = {"workload": {"model": "NVILA-8B shapes, synthetic weights", "llm_layers": a.layers, "micro_batch": b, "positions_per_sample": T // b, "packed_rows": T,
                        "rank": a.rank, "alpha": 16, "tuned": "adapters + mm_projector", "rounds": a.rounds, "steps_per_round": a.steps},
           "steps": steps, "memory": memory}
    if "full_sft" in steps:
        out["a_lora_vs_full"] = {"lora_ms": steps["lora"]["ms"], "full_ms": steps["full_sft"]["ms"], "ratio": round(steps["lora"]["ms"] / steps["full_sft"]["ms"], 4),
                                 "difference_ms": round(steps["full_sft"]["ms"] - steps["lora"]["ms"], 3),
                                 "larger_spread_ms": max(steps["lora"]["spread_ms"], steps["full_sft"]["spread_ms"])}
    out["b_adapters_own_cost"] = {"lora_ms": steps["lora"]["ms"], "zero_targets_ms": steps["lora_zero_targets"]["ms"],
                                  "adapters_ms": round(steps["lora"]["ms"] - steps["lora_zero_targets"]["ms"], 3)}
    sessions.clear()                                                  # the kernels alone: on a quiet device, the trainers' buffers released
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    rows = bench_kernels(cfg.llm, T, a.rank, a.kernel_reps)
    out["c_kernels"] = rows
    out["c_kernels_sum_per_layer_us"] = round(sum(r["us"] * r["uses_per_layer"] for r in rows), 1)
    out["d_memory"] = memory
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "c_kernels"}))
    for r in rows:
        print(f"{r['kernel']:6s} {str(r['shape']):28s} x{r['uses_per_layer']}  {r['us']:8.2f} us (spread {r['spread_us']:.2f})  bytes/8TBs {r['us_at_8TBs']:7.2f} us   {r['where']}")


if __name__ == "__main__":
    main()

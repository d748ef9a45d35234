"""W4A16 batched decode measurements, one process on one GPU:

  for n in 2, 4, 8, 16 sequences of NVILA-8B widths (seeded synthetic weights, 1 x 448^2 image + 512-token prompt per row), ms per step and
  aggregate tokens/s of
    1. the bf16 batched step   (vila_llm_decode_step_batch),
    2. the W4 batched step     (vila_llm_decode_step_batch_w4, quantize_w4(batch_decode=True)),
    3. the solo W4 step        (vila_llm_decode_step_w4, one sequence per weight pass: n sequences served one after another).

    python tools/w4_batch_decode_bench.py [--steps 50] [--layers 28] [--out profiles/w4_batch_decode_bench.json]

Timing: each step is one hipGraph replay (the graph generate() captured); a row is the median over `--iters` timings of `--steps` back-to-back
replays, divided by `--steps`.  Every row decodes from the same 1 image + 512-token contexts (positions advance during the timed replays).

Per-kernel times come from a separate run under rocprofv3 of the W4 batched step alone at one n (`--profile-n N`, NVILA-8B widths, `--layers`
layers: the kernels' shapes do not depend on depth):

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/w4_batch_decode_bench.py --profile-n 8 --layers 4
    python tools/w4_batch_decode_bench.py --kernel-tbs DIR8 DIR16 --out ...     (adds the per-projection TB/s to the JSON)

The trace's gemv_w4_batch_kernel dispatches are told apart by mode and block size (q|k|v mode 2, gate/up mode 1; o_proj and down_proj are both
mode 0, with 4 and 16 waves per block at K = 3584 and 18944).  Bytes per projection = int4 words + scale/zero words + the n activation rows
(`proj_bytes`), computed here.
"""
import argparse
import csv
import glob
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
    return statistics.median(ts)


def batched_ms(llm, e, m, n, steps, iters):
    """ms per batched step for the first n rows (bf16 or W4, whichever the model's batched step is)."""
    max_new = (iters + 1) * steps + 2
    out = llm.generate(inputs_embeds=e[:n], attention_mask=m[:n], max_new_tokens=max_new, eos_token_id=-1)     # session + captured graph
    torch.cuda.synchronize()
    st = llm._bdecode
    assert st is not None and st.graph is not None and out.shape == (n, max_new)
    S = [int(v) for v in m[:n].sum(1).tolist()]
    st.pos.copy_(torch.tensor(S, dtype=torch.int32)); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def solo_ms(llm, e, m, steps, iters):
    max_new = (iters + 1) * steps + 2
    n = int(m[0].sum())
    llm.generate(inputs_embeds=e[:1, :n], max_new_tokens=max_new, eos_token_id=-1)        # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None
    st.pos.fill_(n); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def proj_bytes(c, n):
    """HBM / L2 bytes of one W4 batched projection at n rows: int4 words (K/2 bytes per row) + one {scale, zero} word per row and group +
    the n bf16 activation rows."""
    H, F, hd = c.hidden_size, c.intermediate_size, c.head_dim
    QKV = (c.num_attention_heads + 2 * c.num_key_value_heads) * hd
    shapes = {"qkv": (QKV, H), "o_proj": (H, H), "gate_up": (2 * F, H), "down": (H, F)}
    return {k: N * K // 2 + N * (K // 128) * 4 + n * K * 2 for k, (N, K) in shapes.items()}


def kernel_rows(trace_dir):
    """gemv_w4_batch_kernel dispatches of a rocprofv3 kernel trace -> {projection: [us, ...]}."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel_trace.csv under {trace_dir}"
    out = {"qkv": [], "o_proj": [], "gate_up": [], "down": []}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r.get("Kernel_Name", "")
                if "gemv_w4_batch_kernel" not in name:
                    continue
                mode = name.split("gemv_w4_batch_kernel<")[1][0]
                wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0)
                us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                key = {"2": "qkv", "1": "gate_up"}.get(mode) or ("down" if wg >= 1024 else "o_proj")
                out[key].append(us)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w4_batch_decode_bench.json"))
    ap.add_argument("--profile-n", type=int, default=0, help="only replay the W4 batched step at this n (for a rocprofv3 run)")
    ap.add_argument("--kernel-tbs", nargs=2, metavar=("DIR_N8", "DIR_N16"), help="per-projection TB/s from two rocprofv3 trace dirs")
    a = ap.parse_args()

    if a.kernel_tbs:
        c = configs.nvila_8b().llm
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res["kernels"] = {}
        for n, d in zip((8, 16), a.kernel_tbs):
            rows, byt = kernel_rows(d), proj_bytes(c, n)
            res["kernels"][str(n)] = {k: {"us_median": round(statistics.median(v), 2), "dispatches": len(v), "bytes": byt[k],
                                          "tb_s": round(byt[k] / (statistics.median(v) * 1e-6) / 1e12, 2)} for k, v in rows.items() if v}
            print(json.dumps({"n": n, **res["kernels"][str(n)]}))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return

    if a.profile_n:
        cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, a.profile_n)
        model.llm.quantize_w4(keep_logical=False, batch_decode=True)
        ms = batched_ms(model.llm, e, m, a.profile_n, a.steps, a.iters)
        print(json.dumps({"profile_n": a.profile_n, "layers": a.layers, "w4_batch_ms": round(ms, 4)}))
        return

    cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, max(NS))
    llm = model.llm
    S = int(m[0].sum())
    rows = {}
    for n in NS:
        rows[n] = {"n": n, "bf16_batch_ms": batched_ms(llm, e, m, n, a.steps, a.iters)}
        print(json.dumps(rows[n]), flush=True)
    llm.quantize_w4(keep_logical=False, batch_decode=True)
    solo = solo_ms(llm, e, m, a.steps, a.iters)
    for n in NS:
        r = rows[n]
        r["w4_batch_ms"] = batched_ms(llm, e, m, n, a.steps, a.iters)
        r["w4_solo_ms"] = solo
        for k in ("bf16_batch", "w4_batch"):
            r[k + "_ms"] = round(r[k + "_ms"], 4)
            r[k + "_tok_s"] = round(n * 1e3 / r[k + "_ms"], 1)
        r["w4_solo_ms"] = round(solo, 4)
        r["w4_solo_tok_s"] = round(1e3 / solo, 1)                 # n sequences one after another: the aggregate is the solo rate
        r["w4_batch_over_bf16_batch"] = round(r["w4_batch_ms"] / r["bf16_batch_ms"], 3)
        print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "context": f"1 x 448^2 image + {a.prompt_tokens}-token prompt per row (S={S})",
                      "steps_per_timing": a.steps, "timings": a.iters, "method": "graph replays"},
           "rows": [rows[n] for n in NS]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):                                   # keep per-kernel results of an earlier --kernel-tbs
        old = json.load(open(a.out))
        if "kernels" in old:
            res["kernels"] = old["kernels"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

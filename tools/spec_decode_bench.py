"""Speculative decoding, greedy and sampled, measured in one process on one GPU: the verify step (vila_llm_decode_step_verify and its `_sample`
form, attn_decode.hip bdec_attn_shared_kernel) at NVILA-8B widths with seeded synthetic weights.

  for bf16 and W4, 769 and 8192 cached keys, n = 4 / 8 / 16 rows per step:
    * ms per verify step (one hipGraph replay: draft + forward of n rows + accept),
    * the solo step at that context and the existing batched step at equal n and keys (n rows in n slots), both untouched code,
    * break-even acceptance t_verify / t_solo - 1: accepted drafts per step from which speculation pays,
    * tokens/s in candidate mode at 0 % acceptance (a candidate that is wrong everywhere: 1 token per step) and at 100 % (the candidate is the
      model's own output, recorded by a run that drafts nothing: n tokens per step).  These are the two ends; synthetic weights have no meaningful
      acceptance rate of their own.
    * the sampled arm at temperature 0.2 / top_k 50 / top_p 0.9 (the server's default request): ms per sampled verify step beside the greedy one —
      both sessions alive at once, their timing rounds alternating — the solo SAMPLED step, and the break-even against it.  sample_delta_us is
      sampled minus greedy verify step: what the three sampler launches and the accept cost over the greedy pick and accept.  The batched sampler's
      cost for the same three launches in the batched step is c - a = 50-72 us in profiles/batch_sample_bench.json, printed beside it.

    python tools/spec_decode_bench.py [--steps 10] [--iters 3] [--layers 28] [--out profiles/spec_decode_bench.json]

Timing: HIP events around `--steps` back-to-back replays, warm (one untimed round first), median of `--iters` rounds, divided by `--steps`.  The KV
caches are filled with seeded noise instead of a prefill (a step's time does not depend on the values); the solo step decodes behind a real prefill.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

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


SAMPLING = (0.2, 50, 0.9, 1)                         # temperature / top_k / top_p of the server's default request, a fixed seed
BATCH_SAMPLER_US = (50, 72)                          # c - a of profiles/batch_sample_bench.json: the same three launches in the batched step


def solo_ms(llm, keys, steps, iters, sampled=False):
    room = steps + 2
    g = torch.Generator(device="cuda").manual_seed(keys)
    e = torch.randn((1, keys, llm.lcfg.hidden_size), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16)
    kw = dict(do_sample=True, temperature=SAMPLING[0], top_k=SAMPLING[1], top_p=SAMPLING[2], seed=SAMPLING[3]) if sampled else {}
    llm.generate(inputs_embeds=e, max_new_tokens=room, eos_token_id=-1, **kw)                 # session + captured graph
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
    """-> {"greedy" | "sampled": (ms per step at 0 % acceptance, at 100 %, tokens per step seen at 0 %, at 100 %)}.  Both sessions live on one cache
    (every step writes the K/V rows it reads at or past `keys` before it reads them) and their timing rounds alternate."""
    room = n * steps + n
    cache = llm.new_cache(((keys + room + 255) // 256) * 256)
    noise(cache, keys + n)
    llm._drop_session("_vdecode")
    arms = {}
    for name in ("greedy", "sampled"):
        st = llm._verify_session(cache, n, room, 2, sampled=name == "sampled")
        llm._vdecode = None                              # keep this session alive beside the next one; dropped by hand below
        if st.sampled:
            llm._verify_set_sampling(st, SAMPLING)

        def reset(n_cand, st=st):
            st.pos.fill_(keys); st.n_out.zero_(); st.n_hist.fill_(1); st.token.fill_(17); st.n_cand.fill_(n_cand)
        reset(0)
        _capture(st, lambda st=st: llm.verify_step(cache, st), lambda reset=reset: reset(0))
        # the model's own output from this state: n * steps replays that draft nothing
        reset(0)
        torch.cuda.synchronize()
        replay(st.graph, st.stream, n * steps)
        own = st.out_ids[:n * steps].clone()
        arms[name] = SimpleNamespace(st=st, reset=reset, own=own, ts={0: [], 1: []}, toks={})
    for which in (0, 1):                                 # candidate wrong everywhere / right everywhere
        for a in arms.values():
            a.st.cand[:n * steps].copy_(a.own if which else a.own + 1)
        for it in range(iters + 1):
            for a in arms.values():                      # the arms alternate inside every round
                a.reset(n * steps)
                torch.cuda.synchronize()
                a.ts[which].append(replay(a.st.graph, a.st.stream, steps) / steps)
                a.toks[which] = int(a.st.n_out.item()) / steps
    out = {}
    for name, a in arms.items():
        assert torch.equal(a.st.out_ids[:n * steps], a.own), f"speculation changed the {name} ids"
        out[name] = (statistics.median(a.ts[0][1:]), statistics.median(a.ts[1][1:]), a.toks[0], a.toks[1])
        llm._vdecode = a.st
        llm._drop_session("_vdecode")
    return out


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
            solo_s = solo_ms(llm, keys, a.steps, a.iters, sampled=True)
            for n in NS:
                bat = batched_ms(llm, n, keys, a.steps, a.iters)
                arms = verify_ms(llm, n, keys, a.steps, a.iters)
                v0, v100, t0, t100 = arms["greedy"]
                s0, s100, u0, u100 = arms["sampled"]
                r = {"dtype": dtype, "keys": keys, "n": n, "solo_ms": round(solo, 4), "batched_ms": round(bat, 4), "verify_ms": round(v0, 4),
                     "verify_ms_all_accepted": round(v100, 4), "verify_over_batched": round(v0 / bat, 3), "break_even_accepted_per_step": round(v0 / solo - 1, 3),
                     "solo_tok_s": round(1e3 / solo, 1), "tok_s_0pct": round(t0 * 1e3 / v0, 1), "tok_s_100pct": round(t100 * 1e3 / v100, 1),
                     "tokens_per_step_0pct": t0, "tokens_per_step_100pct": t100,
                     "solo_sampled_ms": round(solo_s, 4), "verify_sampled_ms": round(s0, 4), "verify_sampled_ms_all_accepted": round(s100, 4),
                     "sample_delta_us": round((s0 - v0) * 1e3, 1), "batch_sampler_c_minus_a_us": list(BATCH_SAMPLER_US),
                     "break_even_accepted_per_step_sampled": round(s0 / solo_s - 1, 3), "solo_sampled_tok_s": round(1e3 / solo_s, 1),
                     "sampled_tok_s_0pct": round(u0 * 1e3 / s0, 1), "sampled_tok_s_100pct": round(u100 * 1e3 / s100, 1),
                     "sampled_tokens_per_step_0pct": u0, "sampled_tokens_per_step_100pct": u100}
                rows.append(r)
                print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "HIP events around back-to-back graph replays, warm, median",
                      "break_even_accepted_per_step": "verify_ms / solo_ms - 1", "verify_over_batched": "verify_ms / batched_ms at equal n and keys",
                      "sampling": {"temperature": SAMPLING[0], "top_k": SAMPLING[1], "top_p": SAMPLING[2]},
                      "sample_delta_us": "verify_sampled_ms - verify_ms (0 % acceptance), greedy and sampled rounds alternating in one process",
                      "break_even_accepted_per_step_sampled": "verify_sampled_ms / solo_sampled_ms - 1",
                      "batch_sampler_c_minus_a_us": "range of c - a in profiles/batch_sample_bench.json: the sampler's three launches in the batched step"},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

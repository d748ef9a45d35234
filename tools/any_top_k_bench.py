"""What the any_top_k flag costs and what it buys, one process on one GPU:

  NVILA-8B widths (seeded synthetic weights, 769 cached keys per row: 1 x 448^2 image + a 512-token prompt), bf16 and W4A16, ms per step of
    a. the flagged sampled batched step whose rows all have top_k = 50, against the unflagged sampled step  (the price of the one extra launch),
    b. the flagged step whose rows all have top_k = 0 / top_p = 0.9, and whose rows all have top_k = 1000, each against a's flagged step,
       at n = 2, 8 and 16 rows,
    c. the solo sampled step with top_k = 0 / top_p = 0.9 against top_k = 50 / top_p = 0.9  (what smp_large_kernel costs a step),
    d. aggregate tok/s of n pure top-p requests (top_k = 0, top_p = 0.9) as rows of the flagged step, against the same requests served solo one
       after another — what happens to them without the flag,
    e. the flagged sampled verify step (top_k = 0) at n = 4, 8 and 16 rows against the solo top_k = 0 step, with the accepted drafts per step at
       which speculation breaks even (verify_ms / solo_ms - 1, as profiles/spec_decode_bench.json reports it).

    python tools/any_top_k_bench.py [--steps 20] [--iters 5] [--layers 28] [--out profiles/any_top_k_bench.json]

Timing: each step is one hipGraph replay; a figure is the median over `--iters` timings of `--steps` back-to-back replays, divided by `--steps`,
after one warm-up round; the spread is max - min of those timings.  The sessions that a comparison sets against each other live side by side and
their timing rounds ALTERNATE inside one run, so drift of the clocks hits both.  The caches hold noise: the weights are synthetic, so the logits
have no meaning, and what a sampler costs on them depends little on their values (the radix passes visit every logit whatever it holds)."""
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

NS = (2, 8, 16)
VERIFY_NS = (4, 8, 16)
KEYS = 769
T, P = 0.2, 0.9                                      # the server's default temperature and top_p
ROW_KINDS = (("k50", 50, P), ("k0_p0.9", 0, P), ("k1000", 1000, 1.0))


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


def summary(ts):
    return round(statistics.median(ts), 4), round((max(ts) - min(ts)) * 1e3, 1)


def alternate(arms, steps, iters):
    """arms: {name: (graph, stream, reset)} -> {name: (median ms per step, spread us)}; the arms alternate inside every round, the first round warms up."""
    ts = {name: [] for name in arms}
    for it in range(iters + 1):
        for name, (graph, stream, reset) in arms.items():
            reset()
            torch.cuda.synchronize()
            ms = replay(graph, stream, steps) / steps
            if it:
                ts[name].append(ms)
    return {name: summary(v) for name, v in ts.items()}


def batched(llm, n, steps, iters):
    """The unflagged and the flagged sampled session of n rows side by side: unflagged at top_k 50, flagged at every kind of row."""
    room = steps + 2
    max_ctx = ((KEYS + room + 255) // 256) * 256
    llm._drop_batch_session()
    plain = llm.batch_open(n, max_ctx, room, sampling=True)
    llm._bdecode = None                              # keep this session alive beside the next one; dropped by hand below
    flagged = llm.batch_open(n, max_ctx, room, sampling=True, any_top_k=True)
    assert flagged is not plain and flagged.any_k and not getattr(plain, "any_k", False)
    arms = {}
    for st in (plain, flagged):
        noise(st.cache, KEYS + n)
    def reset_of(st, k, p):
        def reset():
            st.pos.fill_(KEYS); st.n_out.zero_(); st.token.fill_(17)
            for b in range(st.pos.numel()):
                llm._batch_set_sampling(st, b, (T, k, p, 1000 + b))
        return reset
    arms["unflagged_k50"] = (plain.graph, plain.stream, reset_of(plain, 50, P))
    for name, k, p in ROW_KINDS:
        arms["flagged_" + name] = (flagged.graph, flagged.stream, reset_of(flagged, k, p))
    out = alternate(arms, steps, iters)
    llm._drop_batch_session()
    llm._bdecode = plain
    llm._drop_batch_session()
    return out


def solo(llm, steps, iters):
    """The solo sampled sessions with top_k 50 and top_k 0 side by side (one cache: every step writes the K/V row it reads at `KEYS` first)."""
    room = steps + 2
    g = torch.Generator(device="cuda").manual_seed(KEYS)
    e = torch.randn((1, KEYS, llm.lcfg.hidden_size), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16)
    arms, sessions = {}, []
    for name, k in (("solo_k50", 50), ("solo_k0_p0.9", 0)):
        llm.generate(inputs_embeds=e, max_new_tokens=room, eos_token_id=-1, do_sample=True, temperature=T, top_k=k, top_p=P, seed=1)      # session + captured graph
        torch.cuda.synchronize()
        st = llm._decode
        assert st is not None and st.graph is not None and all(st is not s for s in sessions)
        llm._decode = None                           # keep it alive beside the next one
        sessions.append(st)
        def reset(st=st):
            st.pos.fill_(KEYS); st.n_out.zero_()
        arms[name] = (st.graph, st.stream, reset)
    out = alternate(arms, steps, iters)
    for st in sessions:
        llm._decode = st
        llm._drop_decode_session()
    return out


def verify(llm, n, steps, iters):
    """The flagged sampled verify step of n rows at top_k 0, drafting nothing (an empty candidate: the time of a step does not depend on what is accepted)."""
    room = n * steps + n
    cache = llm.new_cache(((KEYS + room + 255) // 256) * 256)
    noise(cache, KEYS + n)
    llm._drop_session("_vdecode")
    st = llm._verify_session(cache, n, room, 2, sampled=True, any_top_k=True)
    assert st.any_k
    llm._verify_set_sampling(st, (T, 0, P, 1))
    def reset():
        st.pos.fill_(KEYS); st.n_out.zero_(); st.n_hist.fill_(1); st.token.fill_(17); st.n_cand.fill_(0)
    reset()
    _capture(st, lambda: llm.verify_step(cache, st), reset)
    out = alternate({"verify": (st.graph, st.stream, reset)}, steps, iters)["verify"]
    llm._drop_session("_vdecode")
    return out


def measure(llm, steps, iters):
    res = {"batched": {}, "verify": {}}
    s = solo(llm, steps, iters)
    res["solo"] = {k: {"ms": v[0], "spread_us": v[1]} for k, v in s.items()}
    res["solo"]["k0_minus_k50_us"] = round((s["solo_k0_p0.9"][0] - s["solo_k50"][0]) * 1e3, 1)
    print(json.dumps({"solo": res["solo"]}), flush=True)
    solo0 = s["solo_k0_p0.9"][0]
    for n in NS:
        b = batched(llm, n, steps, iters)
        r = {k: {"ms": v[0], "spread_us": v[1]} for k, v in b.items()}
        f50 = b["flagged_k50"][0]
        r["a_flagged_k50_minus_unflagged_us"] = round((f50 - b["unflagged_k50"][0]) * 1e3, 1)
        r["b_k0_p0.9_minus_flagged_k50_us"] = round((b["flagged_k0_p0.9"][0] - f50) * 1e3, 1)
        r["b_k1000_minus_flagged_k50_us"] = round((b["flagged_k1000"][0] - f50) * 1e3, 1)
        r["d_rows_tok_s"] = round(n * 1e3 / b["flagged_k0_p0.9"][0], 1)
        r["d_solo_one_after_another_tok_s"] = round(1e3 / solo0, 1)
        r["d_rows_over_solo"] = round(n * solo0 / b["flagged_k0_p0.9"][0], 2)
        res["batched"][f"n{n}"] = r
        print(json.dumps({f"n{n}": r}), flush=True)
    for n in VERIFY_NS:
        ms, spread = verify(llm, n, steps, iters)
        r = {"verify_k0_ms": ms, "spread_us": spread, "solo_k0_ms": solo0, "break_even_accepted_per_step": round(ms / solo0 - 1, 3)}
        res["verify"][f"n{n}"] = r
        print(json.dumps({f"verify_n{n}": r}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "any_top_k_bench.json"))
    a = ap.parse_args()

    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = a.layers
    llm = build_model(cfg, seed=0).llm
    res = {"config": {"model": cfg.name, "layers": a.layers, "vocab": cfg.llm.vocab_size, "keys_per_row": KEYS, "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "graph replays; median of the timings after one warm-up round; spread = max - min of the timings; the sessions of one "
                                "comparison live side by side and alternate inside every round",
                      "rows": f"temperature {T}; k50: top_k 50 / top_p {P}; k0_p0.9: top_k 0 / top_p {P}; k1000: top_k 1000 / top_p 1.0",
                      "a": "flagged session, every row top_k 50, minus the unflagged sampled session: the one extra launch",
                      "b": "flagged session, every row top_k 0 / top_p 0.9 (or top_k 1000), minus a's flagged session",
                      "c": "solo sampled step, top_k 0 / top_p 0.9 minus top_k 50 / top_p 0.9",
                      "d": "n rows of top_k 0 / top_p 0.9 per flagged step (n / step) against the solo top_k 0 step (1 / step): the same requests one after another",
                      "e": "flagged sampled verify step at top_k 0; break_even_accepted_per_step = verify_ms / solo_k0_ms - 1"}}
    for dtype in ("bf16", "w4"):
        if dtype == "w4":
            llm._drop_batch_session()
            llm._drop_decode_session()
            llm.quantize_w4(keep_logical=False, batch_decode=True)
        print(json.dumps({"dtype": dtype}), flush=True)
        res[dtype] = measure(llm, a.steps, a.iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

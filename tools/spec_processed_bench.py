"""What the processing chain costs a verify step (speculative decoding for penalised, constrained and logprob requests), one process on one GPU:

  NVILA-8B widths (seeded synthetic weights), 769 cached keys, bf16 and W4, n = 4 / 8 / 16 rows per step, ms per step (one hipGraph replay) of
    plain   the plain verify step, greedy and sampled (vila_llm_decode_step_verify / _sample: the code path of a build without the feature),
    pen     the processed step with penalties 1.1 / 0.5 / 0.25,
    con     with an automaton (a regex over a synthetic byte vocabulary padded to the model's),
    all     with penalties, the automaton and logprob records,
  each greedy and sampled (temperature 0.2 / top_k 50 / top_p 0.9), all eight sessions alive on one cache and their timing rounds ALTERNATING inside
  the run; the solo penalised / constrained / penalised + constrained + logprob step at the same context, and from it the break-even accepted drafts
  per step, t_processed / t_solo - 1; and the added launches on their own (captured back to back, `--reps` per graph) on [n][vocab] rows.

    python tools/spec_processed_bench.py [--steps 10] [--iters 3] [--layers 28] [--out profiles/spec_processed_bench.json]

Timing: HIP events around `--steps` back-to-back replays, warm (one untimed round first), median of `--iters` rounds, divided by `--steps`; the spread
is max - min of those rounds.  The yardstick of every delta is the plain verify step of the same run.  The KV cache is filled with seeded noise
instead of a prefill (a step's time does not depend on the values); no draft is offered (the graph is fixed: a step's time does not depend on how
many drafts it accepts, profiles/spec_decode_bench.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vila_amd import _lib, configs, ops  # noqa: E402
from vila_amd import constrain as cn  # noqa: E402
from vila_amd._lib import check  # noqa: E402
from vila_amd.modules import _capture  # noqa: E402

NS = (4, 8, 16)
KEYS = 769
SAMPLING = (0.2, 50, 0.9, 1)
PEN = (1.1, 0.5, 0.25)
ARMS = [(kind, sampled) for kind in ("plain", "pen", "con", "all") for sampled in (False, True)]


def replay(graph, stream, steps):
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


def automaton(vocab):
    """A never-ending regex over single bytes and a few pieces, lifted over `vocab` ids (ids 0..255 = the bytes, the rest unusable)."""
    tb = [bytes([i]) for i in range(256)] + [b"yes", b"no", b"12", b"100"] + [None] * (vocab - 260)
    return cn.ConstraintCompiler(tb, (vocab - 1,)).regex(r"(yes|no|ab|abc|bc|[ ,01]|12|100)+")


def med(ts):
    return statistics.median(ts[1:]), max(ts[1:]) - min(ts[1:])


def verify_arms(llm, n, steps, iters, auto):
    """-> {(kind, sampled): (ms per step, spread ms)}"""
    room = steps + n + 2
    cache = llm.new_cache(((KEYS + room + 255) // 256) * 256)
    noise(cache, KEYS + n)
    llm._drop_session("_vdecode")
    caps = llm._constraint_caps(llm.CONSTRAIN_MAX_STATES, llm.CONSTRAIN_MAX_CLASSES)
    arms = {}
    for kind, sampled in ARMS:
        kw = {}
        if kind in ("pen", "all"):
            kw["penalties"] = True
        if kind in ("con", "all"):
            kw["constraints"] = caps
        if kind == "all":
            kw["logprobs"] = True
        st = llm._verify_session(cache, n, room, 2, sampled=sampled, **kw)
        llm._vdecode = None                              # keep this session alive beside the next one; dropped by hand below
        if sampled:
            llm._verify_set_sampling(st, SAMPLING)

        def reset(st=st, kw=kw):
            st.pos.fill_(KEYS); st.n_out.zero_(); st.n_hist.fill_(1); st.token.fill_(17); st.n_cand.fill_(0)
            if "penalties" in kw:
                llm._set_penalties(st, 0, PEN)
            if "constraints" in kw:
                llm._set_constraint(st, 0, auto)
        reset()
        _capture(st, lambda st=st: llm.verify_step(cache, st), reset)
        arms[(kind, sampled)] = (st, reset, [])
    for it in range(iters + 1):
        for st, reset, ts in arms.values():              # the arms alternate inside every round
            reset()
            torch.cuda.synchronize()
            ts.append(replay(st.graph, st.stream, steps) / steps)
    out = {k: med(ts) for k, (st, reset, ts) in arms.items()}
    for st, _, _ in arms.values():
        llm._vdecode = st
        llm._drop_session("_vdecode")
    return out


def solo_ms(llm, steps, iters, auto, kind, sampled):
    g = torch.Generator(device="cuda").manual_seed(KEYS)
    e = torch.randn((1, KEYS, llm.lcfg.hidden_size), device="cuda", generator=g, dtype=torch.float32).mul_(0.02).to(torch.bfloat16)
    kw = dict(do_sample=True, temperature=SAMPLING[0], top_k=SAMPLING[1], top_p=SAMPLING[2], seed=SAMPLING[3]) if sampled else {}
    if kind in ("pen", "all"):
        kw.update(repetition_penalty=PEN[0], presence_penalty=PEN[1], frequency_penalty=PEN[2])
    if kind in ("con", "all"):
        kw.update(constraint=auto)
    if kind == "all":
        kw.update(logprobs=5)
    llm.generate(inputs_embeds=e, max_new_tokens=steps + 2, eos_token_id=-1, **kw)                 # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None
    ts = []
    for it in range(iters + 1):
        st.pos.fill_(KEYS); st.n_out.zero_()
        torch.cuda.synchronize()
        ts.append(replay(st.graph, st.stream, steps) / steps)
    llm._drop_decode_session()
    return med(ts)[0]


def launches_alone_us(n, vocab, auto, reps, iters):
    """us per launch (group) of the added kernels on [n][vocab] rows, `reps` of them captured back to back in one graph."""
    lib = _lib.load()
    dev = "cuda"
    x = torch.randn((n, vocab), device=dev)
    y = torch.empty_like(x)
    S = int(lib.vila_logits_penalize_slices())
    pv, pi = torch.empty((n, S), device=dev), torch.empty((n, S), device=dev, dtype=torch.int32)
    tok = torch.full((n,), 17, device=dev, dtype=torch.int64)
    counts = torch.zeros(vocab, device=dev, dtype=torch.int16)
    p3 = [torch.tensor([v], device=dev) for v in PEN]
    pen = _lib.VilaPenalties(p3[0].data_ptr(), p3[1].data_ptr(), p3[2].data_ptr(), counts.data_ptr(), vocab)
    ld = (vocab + 3) // 4 * 4
    cls = torch.zeros(ld, device=dev, dtype=torch.int16)
    cls[:vocab].copy_(torch.from_numpy(auto.cls.view("int16")).to(dev))
    nxt = torch.from_numpy(auto.next.reshape(-1).copy()).to(dev)
    state = torch.tensor([auto.start], device=dev, dtype=torch.int32)
    nc = torch.tensor([auto.n_classes], device=dev, dtype=torch.int32)
    con = _lib.VilaConstraints(state.data_ptr(), cls.data_ptr(), ld, nxt.data_ptr(), nxt.numel(), nc.data_ptr())
    states = torch.zeros(n, device=dev, dtype=torch.int32)
    m = torch.zeros(1, device=dev, dtype=torch.int32)
    rec = torch.arange(n, device=dev, dtype=torch.int32)
    tl, pl, il = torch.zeros(n, device=dev), torch.zeros((n, 20), device=dev), torch.zeros((n, 20), device=dev, dtype=torch.int32)
    lp = _lib.VilaLogprobOut(tl.data_ptr(), pl.data_ptr(), il.data_ptr(), n)
    ws = torch.empty((lib.vila_logprobs_workspace_bytes(n),), device=dev, dtype=torch.uint8)
    s = lambda: ops._stream()
    calls = {
        "penalize_verify": lambda: check(lib.vila_logits_penalize_verify_f32(x.data_ptr(), vocab, n, vocab, C.byref(pen), tok.data_ptr(), y.data_ptr(), vocab,
                                                                             pv.data_ptr(), pi.data_ptr(), s()), "pen"),
        "constrain_verify (chain + mask)": lambda: check(lib.vila_logits_constrain_verify_f32(x.data_ptr(), vocab, n, vocab, C.byref(con), tok.data_ptr(),
                                                                                              states.data_ptr(), y.data_ptr(), vocab, pv.data_ptr(), pi.data_ptr(),
                                                                                              s()), "con"),
        "commit": lambda: check(lib.vila_verify_commit(C.byref(pen), C.byref(con), vocab, tok.data_ptr(), states.data_ptr(), m.data_ptr(), n, s()), "commit"),
        "logprobs (one sequence, 2 launches)": lambda: check(lib.vila_logprobs_seq_f32(x.data_ptr(), vocab, n, vocab, tok.data_ptr(), 20, rec.data_ptr(),
                                                                                       C.byref(lp), ws.data_ptr(), s()), "lp"),
    }
    out = {}
    stream = torch.cuda.Stream()
    for name, call in calls.items():
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            call()
            stream.synchronize()
            check(lib.vila_graph_begin(stream.cuda_stream), "graph_begin")
            for _ in range(reps):
                call()
            g = C.c_void_p()
            check(lib.vila_graph_end(stream.cuda_stream, C.byref(g)), "graph_end")
            stream.synchronize()
        ts = [replay(g, stream, 1) / reps for _ in range(iters + 1)]
        check(lib.vila_graph_destroy(g), "graph_destroy")
        out[name] = round(med(ts)[0] * 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_processed_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    cfg.llm.num_hidden_layers = a.layers
    llm = build_model(cfg, seed=0).llm
    V = cfg.llm.vocab_size
    auto = automaton(V)
    alone = {n: launches_alone_us(n, V, auto, a.reps, a.iters) for n in NS}
    for n in NS:
        print(json.dumps({"n": n, "launches_alone_us": alone[n]}), flush=True)
    rows = []
    for dtype in ("bf16", "w4"):
        if dtype == "w4":
            llm.quantize_w4(keep_logical=False, batch_decode=True)
        solo = {(kind, sampled): solo_ms(llm, a.steps, a.iters, auto, kind, sampled) for kind, sampled in ARMS}
        for n in NS:
            arms = verify_arms(llm, n, a.steps, a.iters, auto)
            for sampled in (False, True):
                base, base_spread = arms[("plain", sampled)]
                r = {"dtype": dtype, "n": n, "pick": "sampled" if sampled else "greedy", "plain_verify_ms": round(base, 4),
                     "plain_spread_us": round(base_spread * 1e3, 1), "solo_plain_ms": round(solo[("plain", sampled)], 4)}
                for kind in ("pen", "con", "all"):
                    ms, spread = arms[(kind, sampled)]
                    r[f"{kind}_verify_ms"] = round(ms, 4)
                    r[f"{kind}_spread_us"] = round(spread * 1e3, 1)
                    r[f"{kind}_minus_plain_us"] = round((ms - base) * 1e3, 1)
                    r[f"solo_{kind}_ms"] = round(solo[(kind, sampled)], 4)
                    r[f"{kind}_break_even_accepted_per_step"] = round(ms / solo[(kind, sampled)] - 1, 3)
                la = alone[n]
                r["launches_alone_sum_us"] = {"pen": round(la["penalize_verify"] + la["commit"], 1),
                                              "con": round(la["constrain_verify (chain + mask)"] + la["commit"], 1),
                                              "all": round(sum(la.values()), 1)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "vocab": V, "keys": KEYS, "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "HIP events around back-to-back graph replays, warm, median; spread = max - min of the timed rounds; the eight verify "
                                "sessions of a (dtype, n) alternate inside every round",
                      "penalties": list(PEN), "sampling": {"temperature": SAMPLING[0], "top_k": SAMPLING[1], "top_p": SAMPLING[2]},
                      "yardstick": "plain_verify_ms of the same run and pick",
                      "break_even_accepted_per_step": "processed verify ms / solo step ms with the same processing - 1",
                      "launches_alone_us": "per call, `reps` calls captured back to back in one graph, on [n][vocab] rows; the logprob index kernel and "
                                           "the pick's first stage that a processing launch replaces are not in the sums"},
           "launches_alone_us": {str(n): alone[n] for n in NS}, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""What structured output costs a decode step, one process on one GPU:

  NVILA-8B widths (seeded synthetic weights, 1 x 448^2 image + 512-token prompt per row: 769 keys), bf16 and W4, ms per step of
    solo greedy, solo sampled (temperature 0.2 / top_k 50 / top_p 0.9), and the greedy batched step at n = 2, 8 and 16 rows, each
      a. without the flag            (the plain session: vila_llm_decode_step / _sample / _batch, the code path of a build without the feature),
      b. a four-way choice           (the constrained session: vila_llm_decode_step[_batch]_constrained, every row carrying the automaton),
      c. a nested-object JSON schema (the same launches; the automaton is read from device arrays),
  alternating in that order per configuration, over a synthetic 152 064-entry vocabulary (the 256 bytes, JSON pieces, seeded ASCII words).  The host
  compile time of both automata and their state and class counts go into the same file.  The class count of a real Qwen2 vocabulary is NOT measured
  here (no tokenizer files on the build machine): the caps are session arguments for that reason.

    python tools/constrain_bench.py [--steps 50] [--iters 5] [--layers 28] [--dtypes bf16,w4] [--out profiles/constrain_bench.json]

Timing: as tools/penalty_bench.py — each step is one hipGraph replay (the graph generate() captured); a figure is the median over `--iters` timings
of `--steps` back-to-back replays, divided by `--steps`, after one warm-up round; the spread is max - min of those timings.  The baseline of every
delta is case a of the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.penalty_bench import NS, SERVER_DEFAULT, model_and_inputs, time_replays  # noqa: E402
from vila_amd import constrain as cn  # noqa: E402

SCHEMA = {"type": "object", "properties": {"name": {"type": "string", "maxLength": 16}, "answer": {"enum": ["A", "B", "C", "D"]},
                                           "box": {"type": "object", "properties": {"x": {"type": "integer"}, "y": {"type": "integer"},
                                                                                    "tags": {"type": "array", "items": {"type": "string", "maxLength": 8}, "maxItems": 2}}},
                                           "score": {"type": "number"}, "ok": {"type": "boolean"}}}
CHOICE = ["A", "B", "C", "D"]


def synthetic_vocab(V, seed=0):
    """256 single bytes, JSON pieces, seeded ASCII words (with and without a leading space) up to V - 2 entries, two EOS ids (None) at the end."""
    rng = np.random.default_rng(seed)
    tb = [bytes([i]) for i in range(256)] + [b'{"', b'": ', b'", "', b'"}', b'": "', b'true', b'false', b'null', b', ', b'": [', b'], "', b'": {"', b'}, "']
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", dtype=np.uint8)
    seen = set(tb)
    while len(tb) < V - 2:
        w = bytes(rng.choice(letters, size=int(rng.integers(2, 9))))
        w = b" " + w if rng.random() < 0.5 else w
        if w not in seen:
            seen.add(w)
            tb.append(w)
    return tb + [None, None]


def solo_ms(llm, e, m, steps, iters, sampled, con):
    max_new = (iters + 1) * steps + 2
    n = int(m[0].sum())
    sampling = SERVER_DEFAULT + (1000,) if sampled else None
    kw = {} if con is None else dict(constraint=con)
    llm._generate_solo(e[:1, :n], None, max_new, -1, sampling, True, False, None, None, None, **kw)      # session + captured graph
    torch.cuda.synchronize()
    st = llm._decode
    assert st is not None and st.graph is not None and (st.sampling is not None) == sampled and (st.con is not None) == (con is not None)
    st.pos.fill_(n); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def batched_ms(llm, e, m, n, steps, iters, con):
    max_new = (iters + 1) * steps + 2
    kw = {} if con is None else dict(constraint=con)
    out = llm._generate_batch(e[:n], m[:n], max_new, -1, None, use_graph=True, **kw)                     # session + captured graph
    torch.cuda.synchronize()
    st = llm._bdecode
    assert st is not None and st.graph is not None and out.shape == (n, max_new) and (st.con is not None) == (con is not None)
    S = [int(v) for v in m[:n].sum(1).tolist()]
    st.pos.copy_(torch.tensor(S, dtype=torch.int32)); st.n_out.zero_()
    return time_replays(st.graph, st.stream, steps, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--dtypes", default="bf16,w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_bench.json"))
    a = ap.parse_args()

    cfg, model, e, m = model_and_inputs(a.layers, a.prompt_tokens, max(NS))
    llm, V = model.llm, cfg.llm.vocab_size
    tb = synthetic_vocab(V)
    automata, compile_info = {}, {}
    for name, ast in (("choice", lambda: cn.choice(CHOICE)), ("schema", lambda: cn.json_schema(SCHEMA, indent=2))):
        t0 = time.perf_counter()
        automata[name] = cn.compile_automaton(ast(), tb, [V - 2, V - 1], max_table=llm.CONSTRAIN_MAX_STATES * llm.CONSTRAIN_MAX_CLASSES)
        compile_info[name] = {"compile_s": round(time.perf_counter() - t0, 3), "states": automata[name].n_states, "classes": automata[name].n_classes}
        print(json.dumps({name: compile_info[name]}), flush=True)
    cases = (("none", None), ("choice", automata["choice"]), ("schema", automata["schema"]))
    S = int(m[0].sum())
    rows = []
    for dtype in a.dtypes.split(","):
        if dtype == "w4":
            llm.quantize_w4(batch_decode=True)
        configs_ = [("solo_greedy", lambda con: solo_ms(llm, e, m, a.steps, a.iters, False, con)),
                    ("solo_sampled", lambda con: solo_ms(llm, e, m, a.steps, a.iters, True, con))]
        configs_ += [(f"batch_{n}", (lambda con, n=n: batched_ms(llm, e, m, n, a.steps, a.iters, con))) for n in NS]
        for name, run in configs_:
            r = {"dtype": dtype, "config": name}
            for case, con in cases:
                ms, spread = run(con)
                r[f"{case}_ms"] = round(ms, 4)
                r[f"{case}_spread_us"] = round(spread * 1e3, 1)
            r["choice_minus_none_us"] = round((r["choice_ms"] - r["none_ms"]) * 1e3, 1)
            r["schema_minus_none_us"] = round((r["schema_ms"] - r["none_ms"]) * 1e3, 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = {"config": {"model": cfg.name, "layers": a.layers, "vocab": V, "vocabulary": "synthetic: 256 bytes, JSON pieces, seeded ASCII words; two EOS ids",
                      "context": f"1 x 448^2 image + {a.prompt_tokens}-token prompt per row (S={S})", "steps_per_timing": a.steps, "timings": a.iters,
                      "method": "graph replays, median of timings after one warm-up round; spread = max - min of the timings",
                      "solo_sampled": "temperature 0.2, top_k 50, top_p 0.9", "baseline": "none_ms of the same run (the session without the flag)",
                      "note": "the class count of a real Qwen2 vocabulary is not measured here"},
           "automata": compile_info, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

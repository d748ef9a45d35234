"""Per-row sampling inside the batched decode step (vila_sample_batch_f32, vila_llm_decode_step_batch[_w4]_sample, batch_open(sampling=True),
generate(batch_sample=True), ContinuousBatcher(batch_sampled=True)).

The batched sampler makes, for every row at once and from per-row DEVICE parameters, the choice the solo sampler (`ops.sample`, pinned to
HF-executed distributions in tests/test_gpu_sampling.py) makes for one row: the top-64 set under the strict (value, lower index) order is
unique however the selection is cut, and the final stage shares the solo kernel's arithmetic — so tokens and distributions are compared
BIT FOR BIT with the solo operator, greedy rows with `ops.argmax`.  Everything in front of the pick is the greedy batched step, so a step's
logits must be the same bits with or without sampling."""
import os

import numpy as np
import pytest
import torch

from vila_amd import configs, serving, synthetic

pytestmark = pytest.mark.gpu


def _dev(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device="cuda")


def _i64(u):
    u &= 0xFFFFFFFFFFFFFFFF
    return u - (1 << 64) if u >= (1 << 63) else u


def _batch(logits, rows, counters, return_dist=True):
    """rows: per row None (greedy) or (temperature, top_k, top_p, seed)."""
    from vila_amd import ops
    t = _dev([0.0 if r is None else r[0] for r in rows], torch.float32)
    k = _dev([50 if r is None else r[1] for r in rows], torch.int32)
    p = _dev([1.0 if r is None else r[2] for r in rows], torch.float32)
    s = _dev([0 if r is None else _i64(r[3]) for r in rows], torch.int64)
    return ops.sample_batch(logits, t, k, p, s, counter=_dev(counters, torch.int32), return_dist=return_dist)


@pytest.mark.parametrize("V", [300, 4096, 152064])
@pytest.mark.parametrize("n", [1, 2, 7, 16])
def test_batched_sampler_equals_the_solo_sampler_bit_for_bit(n, V):
    from vila_amd import ops
    g = torch.Generator().manual_seed(1000 * n + V)
    logits = (torch.randn(n, V, generator=g) * 3)
    # a row with exact ties: the whole row drawn from 7 values, so the top-64 holds many equal logits and the index decides
    tie_row = n - 1
    logits[tie_row] = torch.randint(0, 7, (V,), generator=g).float() * 0.5
    logits = logits.cuda()
    rows, counters = [], []
    for i in range(n):
        greedy = (i % 4 == 1) or (n > 2 and i == tie_row - 1)
        rows.append(None if greedy else (0.2 + 0.37 * (i % 5), 1 + (i * 13 + V) % 64, (0.3, 0.9, 1.0, 0.55)[i % 4], 0x9E3779B97F4A7C15 * (i + 1) + n))
        counters.append(5 + 97 * i)
    if n >= 7:
        rows[2] = (0.7, 64, 1.0, 3)                                    # the widest candidate set
        rows[4] = (1.3, 1, 0.9, 4)                                     # top_k 1: the largest key whatever the draw
    tok, dist, ids = _batch(logits, rows, counters)
    assert tok.shape == (n,) and dist.shape == (n, 64) and ids.shape == (n, 64)
    for i, r in enumerate(rows):
        if r is None:
            want = ops.argmax(logits[i])
            assert int(tok[i]) == int(want), (i, int(tok[i]), int(want))
            assert float(dist[i, 0]) == 1.0 and int(ids[i, 0]) == int(want) and float(dist[i, 1:].abs().sum()) == 0 and bool((ids[i, 1:] == -1).all())
        else:
            w_tok, w_dist, w_ids = ops.sample(logits[i], r[0], r[1], r[2], r[3], counter=_dev([counters[i]], torch.int32), return_dist=True)
            assert int(tok[i]) == int(w_tok), (i, r, int(tok[i]), int(w_tok))
            assert torch.equal(ids[i], w_ids), (i, r)
            assert torch.equal(dist[i].view(torch.int32), w_dist.view(torch.int32)), (i, r, float((dist[i] - w_dist).abs().max()))
    # ties go to the lower index in a greedy row as well: the tie row's argmax is the first index of its maximum
    first_max = int((logits[tie_row] == logits[tie_row].max()).nonzero()[0])
    t2, _, _ = _batch(logits, [None] * n, counters)
    assert int(t2[tie_row]) == first_max
    # rows of a strided view (the batched step's logits buffer may be wider than the vocabulary in use)
    if V == 4096 and n == 7:
        wide = torch.zeros((n, V + 64), device="cuda")
        wide[:, :V] = logits
        wide[:, V:] = 1e9                                              # beyond the vocabulary: must never be read
        t3, d3, i3 = _batch(wide[:, :V], rows, counters)
        assert torch.equal(t3, tok) and torch.equal(i3, ids) and torch.equal(d3, dist)
    # deterministic run to run
    t4, d4, i4 = _batch(logits, rows, counters)
    assert torch.equal(t4, tok) and torch.equal(d4, dist) and torch.equal(i4, ids)


def test_batched_sampler_matches_the_hf_executed_fixture():
    """The six cases of tests/golden/sampling_hf.npz whose top_k the batched path serves (c0-c5; c6-c9 have top_k 100 / 1000 / 0 / 5000): the
    case's parameters on one row of a batch whose other rows use other parameters on the same logits.  Bound: the fixture's own 2e-5
    (test_sampler_matches_the_hf_executed_fixture); the other rows against the oracle's restatement of the HF chain, same bound."""
    from oracle import vila_oracle as O
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampling_hf.npz"))
    others = [(0.9, 40, 0.3, 11), None, (1.5, 1, 0.9, 12), (0.2, 50, 0.9, 13), (0.7, 64, 0.5, 14)]
    done = 0
    for c in range(10):
        if f"c{c}_params" not in fx:
            break
        V, temperature, top_k, top_p = fx[f"c{c}_params"]
        if not 1 <= int(top_k) <= 64:
            continue
        logits1 = torch.from_numpy(fx[f"c{c}_logits"]).float()
        ref = torch.from_numpy(fx[f"c{c}_probs"])
        where = c % 6
        rows = list(others)
        rows.insert(where, (float(temperature), int(top_k), float(top_p), c))
        logits = logits1[None].repeat(len(rows), 1).contiguous().cuda()
        tok, dist, ids = _batch(logits, rows, list(range(len(rows))))
        for i, r in enumerate(rows):
            if r is None:
                assert int(tok[i]) == int(logits1.argmax())
                continue
            want = ref if i == where else O.sample_distribution(logits1, r[0], r[1], r[2])
            got = torch.zeros(int(V), dtype=torch.float64)
            valid = ids[i] >= 0
            got[ids[i][valid].long().cpu()] = dist[i][valid].double().cpu()
            err = float((got - want).abs().max())
            assert err < 2e-5, (c, i, r, err)
            assert float(want[int(tok[i])]) > 0
        done += 1
    assert done == 6


def test_batched_draws_follow_the_distribution():
    """The set-up of test_draws_follow_the_distribution_and_the_counter_drives_the_stream (V = 4096, 0.8 / 20 / 0.95, 4000 draws), drawn as 250
    batch calls of 16 rows that share logits and parameters and differ in seed; the counter changes per call.  chi2 < 60 over <= 20 cells."""
    from oracle import vila_oracle as O
    from vila_amd import ops
    V, n, calls = 4096, 16, 250
    logits1 = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 2
    ref = O.sample_distribution(logits1, 0.8, 20, 0.95)
    logits = logits1[None].repeat(n, 1).contiguous().cuda()
    t, k, p = _dev([0.8] * n, torch.float32), _dev([20] * n, torch.int32), _dev([0.95] * n, torch.float32)
    seeds = [1234 + 7919 * i for i in range(n)]
    s = _dev(seeds, torch.int64)
    ctr = torch.zeros(n, dtype=torch.int32, device="cuda")
    draws = []
    for c in range(calls):
        ctr.fill_(c)
        draws.append(ops.sample_batch(logits, t, k, p, s, counter=ctr))
    draws = torch.stack(draws).cpu()                                   # [calls, n]
    counts = torch.zeros(V, dtype=torch.float64)
    counts.index_add_(0, draws.reshape(-1), torch.ones(calls * n, dtype=torch.float64))
    support = ref > 0
    assert int(support.sum()) <= 20
    assert float(counts[~support].sum()) == 0                          # never outside top-k / nucleus
    exp = ref[support] * (calls * n)
    chi2 = float(((counts[support] - exp) ** 2 / exp).sum())
    print(f"batched draws: chi2 = {chi2:.2f} over {int(support.sum())} cells")
    assert chi2 < 60, chi2
    # the same (seed, counter) gives the same token whichever row it sits in — and it is the solo sampler's token
    perm = [(i * 5 + 3) % n for i in range(n)]
    ctr.fill_(7)
    moved = ops.sample_batch(logits, t, k, p, _dev([seeds[j] for j in perm], torch.int64), counter=ctr).cpu()
    assert moved.tolist() == [int(draws[7, j]) for j in perm]
    assert int(ops.sample(logits[0], 0.8, 20, 0.95, seed=seeds[3], counter=ctr[:1])) == int(draws[7, 3])


def test_batched_sampler_refuses_what_it_cannot_serve():
    from vila_amd import ops
    lg = torch.randn(17, 500).cuda()
    t, k, p, s = _dev([1.0] * 17, torch.float32), _dev([5] * 17, torch.int32), _dev([1.0] * 17, torch.float32), _dev([0] * 17, torch.int64)
    with pytest.raises(ValueError):
        ops.sample_batch(lg, t, k, p, s)                               # more than 16 rows
    with pytest.raises(ValueError):
        ops.sample_batch(lg[:4], t[:3], k[:4], p[:4], s[:4])           # a parameter array of another length
    # a bad device value is clamped, never an out-of-range index: top_k 0 / 1000 behave as 1 / 64, top_p 7 as 1
    lg4 = lg[:4].contiguous()
    tok, dist, ids = ops.sample_batch(lg4, t[:4], _dev([0, 1000, 64, 1], torch.int32), _dev([7.0, 1.0, 1.0, 1.0], torch.float32), s[:4], return_dist=True)
    assert int(tok[0]) == int(lg4[0].argmax()) and int((ids[0] >= 0).sum()) == 1 and int((ids[1] >= 0).sum()) == 64
    assert torch.equal(ids[1], ops.sample(lg4[1], 1.0, 64, 1.0, 0, return_dist=True)[2])


# ----------------------------------------------------------------------------------------------------------------------
# the step
# ----------------------------------------------------------------------------------------------------------------------
def _tiny(seed, w4):
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    if w4:
        cfg.llm.intermediate_size = 1152                               # K of down_proj: a multiple of the 128-wide quantisation group
    model = build_model(cfg, seed=seed)
    if w4:
        model.llm.quantize_w4(batch_decode=True)
    g = torch.Generator().manual_seed(seed)
    L = 20
    ids = torch.randint(0, 900, (3, L), generator=g)
    mask = torch.ones(3, L, dtype=torch.bool); mask[1, 13:] = False; mask[2, 5:] = False
    e = model.llm.embed_tokens(ids.cuda())
    return cfg, model, e, mask.cuda(), [20, 13, 5]


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_sampled_batched_step_picks_like_the_solo_sampler_and_leaves_the_logits_alone(w4):
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(31, w4)
    llm = model.llm
    n_new, seed = 9, 4242
    kw = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95)
    forced = torch.randint(0, 900, (3, n_new), generator=torch.Generator().manual_seed(7))
    ids, lg = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=-1, seed=seed, batch_sample=True,
                           return_logits=True, forced_ids=forced, use_graph=False, **kw)
    assert llm._bdecode is not None and llm._bdecode.sampling, "the sampled batch did not take the batched step"
    assert ids.shape == (3, n_new) and lg.shape == (n_new, 3, cfg.llm.vocab_size)
    for b in range(3):
        for t in range(n_new):
            ctr = _dev([lens[b] - 1 + t], torch.int32)                 # the position of the token the step consumed (prefill row: S - 1)
            want = ops.sample(lg[t, b].contiguous(), kw["temperature"], kw["top_k"], kw["top_p"], seed + b, counter=ctr)
            assert int(ids[b, t]) == int(want), (b, t, int(ids[b, t]), int(want))
    assert len({tuple(r) for r in ids.tolist()}) > 1
    # the pick is the only difference: the greedy batched step fed the same ids returns the same logits, bit for bit
    _, lg_greedy = llm._generate_batch(e, mask, n_new, -1, None, use_graph=False, forced_ids=forced, return_logits=True)
    assert not llm._bdecode.sampling
    assert torch.equal(lg_greedy.view(torch.int32), lg.view(torch.int32))
    # without the opt-in a sampled batch keeps today's row-by-row route
    llm._drop_batch_session()
    rows = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=4, eos_token_id=-1, seed=seed, **kw)
    assert llm._bdecode is None and rows.shape == (3, 4)
    # top_k outside 1..64 is not served by the batched step even with the opt-in
    llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=3, eos_token_id=-1, seed=seed, batch_sample=True, do_sample=True, top_k=100)
    assert llm._bdecode is None


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_sampled_batch_graph_equals_eager_and_survives_a_change_of_parameters(w4):
    cfg, model, e, mask, lens = _tiny(33, w4)
    llm = model.llm
    n_new = 12
    kw = dict(max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=30, top_p=0.95, batch_sample=True, attention_mask=mask)
    g = llm.generate(inputs_embeds=e, seed=77, use_graph=True, **kw)
    sess, graph = llm._bdecode, llm._bdecode.graph
    assert sess.sampling and graph is not None and g.shape == (3, n_new)
    eg = llm.generate(inputs_embeds=e, seed=77, use_graph=False, **kw)
    assert torch.equal(g, eg)
    assert torch.equal(llm.generate(inputs_embeds=e, seed=77, use_graph=True, **kw), g)
    other = llm.generate(inputs_embeds=e, seed=1077, use_graph=True, **dict(kw, temperature=1.4))
    assert llm._bdecode is sess and llm._bdecode.graph is graph, "other seeds / temperatures re-captured the batched graph"
    assert all(not torch.equal(other[b], g[b]) for b in range(3))
    # per-row parameters: change row 1 only (seed and temperature), make row 2 greedy — row 0 keeps its ids, the graph stays
    base = [(0.9, 30, 0.95, 77 + b) for b in range(3)]
    mixed = llm._generate_batch(e, mask, n_new, -1, None, use_graph=True, sampling=[base[0], (1.7, 64, 1.0, 5), None])
    assert llm._bdecode is sess and llm._bdecode.graph is graph
    assert torch.equal(mixed[0], g[0]) and not torch.equal(mixed[1], g[1])
    assert torch.equal(llm._generate_batch(e, mask, n_new, -1, None, use_graph=False, sampling=[base[0], (1.7, 64, 1.0, 5), None]), mixed)
    # a greedy row inside a sampling session == the same row of the batch in a greedy session
    all_greedy = llm._generate_batch(e, mask, n_new, -1, None, use_graph=True, sampling=[None, None, None])
    assert llm._bdecode is sess and llm._bdecode.graph is graph
    greedy = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=-1)
    assert not llm._bdecode.sampling
    assert torch.equal(all_greedy, greedy) and torch.equal(mixed[2], greedy[2])
    assert not torch.equal(g, greedy)                                  # it really samples
    # host-side validation where the values are known
    st = llm.batch_open(3, 256, 16, sampling=True)
    assert st.sampling and True in st.key[:4]
    for bad in ((0.0, 50, 0.9, 1), (0.5, 0, 0.9, 1), (0.5, 65, 0.9, 1), (0.5, -1, 0.9, 1), (0.5, 50, 0.0, 1), (0.5, 50, 1.5, 1)):
        with pytest.raises(ValueError):
            llm.batch_admit(st, 0, e[2, :5], sampling=bad)
    with pytest.raises(ValueError):
        llm.batch_admit(llm.batch_open(3, 256, 16), 0, e[2, :5], sampling=(0.5, 50, 0.9, 1))       # a greedy session takes no sampled row
    # batch_open / admit / run / release: a sampled row beside a greedy one; ONE session and graph for every mix; released rows fall back to greedy
    def rows_of(st, sampling1):
        llm.batch_release(st, [0, 1, 2])
        f0 = llm.batch_admit(st, 0, e[0, :20])
        f1 = llm.batch_admit(st, 1, e[1, :13], sampling=sampling1) if sampling1 is not None else llm.batch_admit(st, 1, e[1, :13])
        llm.batch_run(st, n_new - 1)
        assert st.n_out.tolist()[:2] == [n_new - 1] * 2 and st.pos.tolist()[:2] == [20 + n_new - 1, 13 + n_new - 1]
        return [f0] + st.out_ids[0, :n_new - 1].tolist(), [f1] + st.out_ids[1, :n_new - 1].tolist()
    st = llm.batch_open(3, 256, 16, sampling=True)
    graph = st.graph
    a0, a1 = rows_of(st, (1.7, 64, 1.0, 78))
    assert st.s_temperature.tolist() == pytest.approx([0.0, 1.7, 0.0]) and st.s_top_k.tolist()[1] == 64 and st.s_seed.tolist()[1] == 78
    b0, b1 = rows_of(st, (1.7, 64, 1.0, 79))
    c0, c1 = rows_of(st, (1.7, 64, 1.0, 78))
    d0, d1 = rows_of(st, None)
    assert llm.batch_open(3, 256, 16, sampling=True) is st and st.graph is graph
    assert a0 == b0 == c0 == d0 and a1 == c1 and a1 != b1 and a1 != d1
    llm.batch_release(st, [1])
    assert st.s_temperature.tolist() == [0.0, 0.0, 0.0]
    stg = llm.batch_open(3, 256, 16)
    assert stg is not st and not stg.sampling
    g0, g1 = rows_of(stg, None)
    assert g0 == a0 and g1 == d1                                       # greedy rows: the same ids in a sampling and in a greedy session


# ----------------------------------------------------------------------------------------------------------------------
# continuous batching
# ----------------------------------------------------------------------------------------------------------------------
def test_continuous_batching_admits_a_sampled_request_beside_a_greedy_row():
    pytest.importorskip("fastapi")
    import time as _t
    from fastapi.testclient import TestClient
    from tests.test_gpu_serving import _image, _tokenizer
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 12).items()}
    model = build_model(cfg, weights=w)
    tok = _tokenizer(cfg)
    img = _image()

    def experiment(seed, batch_sampled=True):
        eng = serving.HipBatchEngine(model, tok, n_slots=4, max_new_tokens=64, eos_token_id=-1, sampling=batch_sampled)
        cb = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, batch_sampled=batch_sampled)
        try:
            fa = cb.submit([img, "describe the image"], 48)            # long, greedy
            while not any(ev[0] == "run" for ev in cb.events):
                _t.sleep(0.001)
            fb = cb.submit("what is this ?", 8, temperature=0.9, top_p=0.95, top_k=30, seed=seed)
            tb, ta = fb.result(timeout=120), fa.result(timeout=120)
            return ta, tb, list(cb.events)
        finally:
            cb.close()

    ta, tb, ev = experiment(5)
    admits = [x for x in ev if x[0] == "admit"]
    assert len(admits) == 2 and admits[1][2] > 0 and admits[1][3] == 1, admits      # the sampled request joined while the greedy row ran
    assert not any(x[0] == "solo" for x in ev)
    assert isinstance(ta, str) and ta and isinstance(tb, str)
    ta2, tb2, _ = experiment(5)
    assert (ta2, tb2) == (ta, tb)                                      # same seed: the same replies
    replies = {experiment(s)[1] for s in (6, 7, 8)}
    assert replies != {tb}                                             # other seeds: other replies
    ta0, tb0, ev0 = experiment(5, batch_sampled=False)
    assert ta0 == ta                                                   # the greedy request is served exactly as without the switch
    assert any(x[0] == "solo" for x in ev0) and isinstance(tb0, str)
    # the endpoint: a request without `temperature` (0.2 / 0.9, top_k 50) is a row, not a solo run
    app = serving.create_app(model, tok, model_name="NVILA-tiny", batch_window_s=0.01, max_batch=4, batch_sampled=True)
    cb = app.state.batcher
    try:
        assert isinstance(cb, serving.ContinuousBatcher) and cb.batch_sampled
        r = TestClient(app).post("/chat/completions", json={"model": "NVILA-tiny", "max_tokens": 5, "messages": [{"role": "user", "content": "what is this ?"}]})
        assert r.status_code == 200, r.text
        assert isinstance(r.json()["choices"][0]["message"]["content"][0]["text"], str)
        assert not any(x[0] == "solo" for x in cb.events) and any(x[0] == "admit" for x in cb.events)
        assert model.llm._bdecode is not None and model.llm._bdecode.sampling
    finally:
        cb.close()


# ----------------------------------------------------------------------------------------------------------------------
# full size
# ----------------------------------------------------------------------------------------------------------------------
def test_full_size_sampled_batch_of_eight():
    """NVILA-8B shapes, 8 rows (1 x 448^2 image + 512-token prompt each), vocabulary 152064, the server's default 0.2 / 50 / 0.9: 16
    graph-replayed steps; the last step's ids equal `ops.sample` on that step's logits, every id lies inside the vocabulary."""
    from vila_amd import ops
    from vila_amd.vlm import build_model
    cfg = configs.nvila_8b()
    model = build_model(cfg, seed=3)
    n, steps, seed = 8, 16, 11
    px = synthetic.make_pixels(cfg, n, 3, device="cuda", dtype=torch.bfloat16)
    ids = torch.stack([synthetic.make_prompt(cfg, 512, 1, 3 + i) for i in range(n)], 0).cuda()
    e, _, m = model._embed(ids, {"image": [px[i] for i in range(n)]})
    llm = model.llm
    out = llm.generate(inputs_embeds=e, attention_mask=m, max_new_tokens=steps + 1, eos_token_id=-1, do_sample=True, temperature=0.2, top_k=50, top_p=0.9,
                       seed=seed, batch_sample=True, use_graph=True)
    st = llm._bdecode
    assert st is not None and st.sampling and st.graph is not None and out.shape == (n, steps + 1)
    assert cfg.llm.vocab_size == 152064 and int(out.min()) >= 0 and int(out.max()) < cfg.llm.vocab_size
    assert st.n_out.tolist() == [steps] * n
    pos = st.pos.tolist()
    for b in range(n):
        want = ops.sample(st.logits[b], 0.2, 50, 0.9, seed + b, counter=_dev([pos[b] - 1], torch.int32))
        assert int(out[b, -1]) == int(want), (b, int(out[b, -1]), int(want))
    again = llm.generate(inputs_embeds=e, attention_mask=m, max_new_tokens=steps + 1, eos_token_id=-1, do_sample=True, temperature=0.2, top_k=50, top_p=0.9,
                         seed=seed, batch_sample=True, use_graph=True)
    assert torch.equal(again, out) and llm._bdecode is st

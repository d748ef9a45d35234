"""Any top_k for the rows of the batched sampler (vila_sample_batch_any_f32, vila_llm_decode_step_batch_any_k, vila_llm_decode_step_verify_any_k;
ops.sample_batch(any_top_k=True), batch_open / generate / HipBatchEngine / ContinuousBatcher(any_top_k=True)).

A row with top_k = 0 (no top-k filter) or top_k > 64 is drawn by the body of the solo sampler's exact kernel, one block per row, from per-row DEVICE
parameters.  The arithmetic is shared, so every comparison with the solo operator (`ops.sample`, pinned to HF-executed distributions in
tests/test_gpu_sampling.py) is an EQUALITY of ids or of bits; everything in front of the pick is the plain batched step, so a step's logits are the
same bits with or without the flag.  Only the HF fixture is compared within a bound, the fixture's own 2e-5."""
import os

import numpy as np
import pytest
import torch

from tests.penalty_ref import counts_of, penalize_ref
from tests.test_gpu_batch_sampling import _batch, _dev, _i64, _tiny
from vila_amd import serving

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _large(r):
    return r is not None and (r[1] == 0 or r[1] > 64)


def _any(logits, rows, counters, dist=False, dense=True):
    """`ops.sample_batch(any_top_k=True)`; rows: per row None (greedy) or (temperature, top_k, top_p, seed)."""
    from vila_amd import ops
    t = _dev([0.0 if r is None else r[0] for r in rows], torch.float32)
    k = _dev([50 if r is None else r[1] for r in rows], torch.int32)
    p = _dev([1.0 if r is None else r[2] for r in rows], torch.float32)
    s = _dev([0 if r is None else _i64(r[3]) for r in rows], torch.int64)
    return ops.sample_batch(logits, t, k, p, s, counter=_dev(counters, torch.int32), return_dist=dist, any_top_k=True, return_dense=dense)


def _solo(row, r, counter, dist=False):
    from vila_amd import ops
    if r is None:
        return ops.argmax(row.contiguous())
    return ops.sample(row.contiguous(), r[0], r[1], r[2], r[3], counter=_dev([counter], torch.int32), return_dist=dist)


MIXED = [None, (0.8, 20, 0.95, 11), (1.1, 64, 1.0, 12), (1.1, 65, 1.0, 13), (0.7, 0, 0.9, 14), (1.3, 100, 1.0, 15), (0.9, 5000, 0.97, 16), (1.0, 0, 1.0, 17)]


def _check_against_solo(logits, rows, counters, tok, dense):
    for i, r in enumerate(rows):
        if _large(r):
            w_tok, w_dense, _ = _solo(logits[i], r, counters[i], dist=True)
            assert int(tok[i]) == int(w_tok), (i, r, int(tok[i]), int(w_tok))
            assert torch.equal(_bits(dense[i]), _bits(w_dense)), (i, r, float((dense[i] - w_dense).abs().max()))
        else:
            assert int(tok[i]) == int(_solo(logits[i], r, counters[i])), (i, r)


@pytest.mark.parametrize("V", [1000, 1025, 152064])
def test_mixed_rows_equal_the_solo_sampler_bit_for_bit(V):
    """Greedy, k = 20, k = 64 | 65 (the two sides of the boundary), k = 0 with p = 0.9, k = 100, k = 5000, k = 0 with p = 1 in ONE call; V = 1000:
    fewer logits than the block has threads, 1025: the last threads' chunk of the index-order draw is empty, 152064: the real vocabulary."""
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(8, V, generator=g) * 3).cuda()
    counters = list(range(8))
    tok, dense = _any(logits, MIXED, counters)
    assert tok.shape == (8,) and dense.shape == (8, V)
    _check_against_solo(logits, MIXED, counters, tok, dense)
    assert any(int(tok[i]) != int(logits[i].argmax()) for i in range(8) if _large(MIXED[i])), "no large row drew anything but its argmax"
    # a row depends neither on its place nor on its neighbours: permuting the rows permutes the tokens and the distributions
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    tok_p, dense_p = _any(logits[perm].contiguous(), [MIXED[j] for j in perm], [counters[j] for j in perm])
    assert tok_p.tolist() == [int(tok[j]) for j in perm]
    assert torch.equal(_bits(dense_p), _bits(dense[perm]))
    # ... nor on n: the large rows alone
    big = [i for i in range(8) if _large(MIXED[i])]
    tok_b, _ = _any(logits[big].contiguous(), [MIXED[j] for j in big], [counters[j] for j in big])
    assert tok_b.tolist() == [int(tok[j]) for j in big]
    # deterministic run to run
    tok2, dense2 = _any(logits, MIXED, counters)
    assert torch.equal(tok2, tok) and torch.equal(_bits(dense2), _bits(dense))


def test_one_row_and_sixteen_large_rows():
    V = 4097
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(16, V, generator=g) * 2.5).cuda()
    rows = [((0.6, 1.0, 1.7)[i % 3], (0, 65, 300, 4096, 4097, 9000)[i % 6], (0.9, 1.0, 0.5, 0.999)[i % 4], 0x9E3779B97F4A7C15 * (i + 1)) for i in range(16)]
    counters = [3 + 101 * i for i in range(16)]
    tok, dense = _any(logits, rows, counters)
    _check_against_solo(logits, rows, counters, tok, dense)
    for i in (0, 4):
        t1, d1 = _any(logits[i:i + 1], rows[i:i + 1], counters[i:i + 1])
        assert int(t1[0]) == int(tok[i]) and torch.equal(_bits(d1[0]), _bits(dense[i]))


def test_padded_row_stride_reads_nothing_beyond_the_vocabulary():
    V, pad = 1025, 37
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(8, V, generator=g) * 3).cuda()
    wide = torch.empty((8, V + pad), device="cuda")
    wide[:, :V] = logits
    wide[:, V:] = float("inf")
    wide[::2, V::2] = float("nan")
    counters = list(range(8))
    tok, dense = _any(logits, MIXED, counters)
    tok_w, dense_w = _any(wide[:, :V], MIXED, counters)
    assert wide[:, :V].stride(0) == V + pad
    assert torch.equal(tok_w, tok) and torch.equal(_bits(dense_w), _bits(dense))


def test_rows_of_1_to_64_and_greedy_rows_keep_their_bits_and_the_unflagged_clamp_holds():
    from vila_amd import ops
    V = 3000
    g = torch.Generator().manual_seed(13)
    logits = (torch.randn(7, V, generator=g) * 3).cuda()
    rows = [None, (0.8, 20, 0.95, 1), (1.1, 64, 1.0, 2), (0.3, 1, 0.9, 3), None, (1.9, 50, 0.4, 4), (1.0, 33, 1.0, 5)]
    counters = [11 * i for i in range(7)]
    tok, dist, ids = _batch(logits, rows, counters)
    tok_a, dist_a, ids_a = _any(logits, rows, counters, dist=True, dense=False)
    assert torch.equal(tok_a, tok) and torch.equal(_bits(dist_a), _bits(dist)) and torch.equal(ids_a, ids)
    # beside large rows they keep them as well, and a large row's 64-slot entries are zeros and -1 ids
    rows2 = rows[:3] + [(0.7, 0, 0.9, 9)] + rows[4:6] + [(1.2, 1000, 1.0, 10)]
    tok_b, dist_b, ids_b, dense_b = _any(logits, rows2, counters, dist=True)
    for i in (0, 1, 2, 4, 5):
        assert int(tok_b[i]) == int(tok[i]) and torch.equal(_bits(dist_b[i]), _bits(dist[i])) and torch.equal(ids_b[i], ids[i])
        assert float(dense_b[i].abs().sum()) == 0.0                    # the dense rows of the other kinds are not written
    for i in (3, 6):
        assert float(dist_b[i].abs().sum()) == 0.0 and bool((ids_b[i] == -1).all())
        assert int(tok_b[i]) == int(_solo(logits[i], rows2[i], counters[i]))
    # without the flag the device clamp is what it was: top_k 0 / 1000 behave as 1 / 64
    t4 = _dev([1.0] * 4, torch.float32)
    tk, dk, ik = ops.sample_batch(logits[:4].contiguous(), t4, _dev([0, 1000, 64, 1], torch.int32), _dev([1.0] * 4, torch.float32), _dev([0] * 4, torch.int64),
                                  return_dist=True)
    assert int(tk[0]) == int(logits[0].argmax()) and int((ik[0] >= 0).sum()) == 1 and int((ik[1] >= 0).sum()) == 64
    # a negative device top_k is clamped to 1 with the flag too
    tn, _ = _any(logits[:2].contiguous(), [(1.0, -3, 1.0, 1), (1.0, -1, 0.5, 2)], [0, 1])
    assert tn.tolist() == [int(logits[0].argmax()), int(logits[1].argmax())]


def test_large_rows_match_the_hf_executed_fixture():
    """Cases c6 - c9 of tests/golden/sampling_hf.npz (k = 100, 1000, 0, 5000 on V = 8192, 20000, 6000, 3000) as four rows of ONE call.  The rows have
    one width, 20000; a shorter case is padded with -inf, which HF's chain gives probability exactly 0 wherever the filters leave it (exp(-inf) = 0;
    with k < V the pads sort last and are cut, with k = 0 or k >= V they stay in the set with zero mass), so the case's distribution is unchanged.
    Bound: 2e-5, what test_gpu_sampling.py applies to the same cases solo; the token lies in the support."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampling_hf.npz"))
    cases = [6, 7, 8, 9]
    W = max(int(fx[f"c{c}_params"][0]) for c in cases)
    logits = torch.full((4, W), float("-inf"))
    rows = []
    for i, c in enumerate(cases):
        V, temperature, top_k, top_p = fx[f"c{c}_params"]
        logits[i, :int(V)] = torch.from_numpy(fx[f"c{c}_logits"]).float()
        rows.append((float(temperature), int(top_k), float(top_p), c))
    assert [r[1] for r in rows] == [100, 1000, 0, 5000]
    tok, dense = _any(logits.cuda(), rows, [0, 1, 2, 3])
    for i, c in enumerate(cases):
        V = int(fx[f"c{c}_params"][0])
        ref = torch.from_numpy(fx[f"c{c}_probs"]).double()
        got = dense[i].double().cpu()
        err = float((got[:V] - ref).abs().max())
        print(f"c{c}: max |p - p_hf| = {err:.3e}")
        assert err < 2e-5, (c, err)
        assert float(got[V:].abs().sum()) == 0.0
        assert int(tok[i]) < V and float(ref[int(tok[i])]) > 0, (c, int(tok[i]))


def test_masked_row_draws_one_of_the_finite_entries():
    V = 1000
    logits = torch.full((2, V), float("-inf"))
    logits[0, [5, 400, 999]] = torch.tensor([0.3, 0.1, 0.2])
    logits[1] = torch.randn(V, generator=torch.Generator().manual_seed(3))
    logits = logits.cuda()
    seen = set()
    for c in range(12):
        rows = [(1.5, 0, 1.0, 21), (1.0, 0, 0.9, 22)]
        tok, _ = _any(logits, rows, [c, c])
        assert int(tok[0]) in (5, 400, 999) and int(tok[0]) == int(_solo(logits[0], rows[0], c))
        seen.add(int(tok[0]))
    assert len(seen) > 1


# ----------------------------------------------------------------------------------------------------------------------
# the steps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_flagged_batched_step_picks_like_the_solo_sampler_and_leaves_the_logits_alone(w4):
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(71, w4)
    llm = model.llm
    assert cfg.llm.vocab_size >= 900
    n_new, seed = 8, 4242
    forced = torch.randint(0, 900, (3, n_new), generator=torch.Generator().manual_seed(7))
    lg_first = None
    for top_k, top_p in ((0, 0.9), (100, 1.0)):
        kw = dict(do_sample=True, temperature=0.9, top_k=top_k, top_p=top_p)
        ids, lg = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=-1, seed=seed, batch_sample=True, any_top_k=True,
                               return_logits=True, forced_ids=forced, use_graph=False, **kw)
        st = llm._bdecode
        assert st is not None and st.sampling and st.any_k and "any_top_k" in st.key, "the batch did not take the flagged batched step"
        assert ids.shape == (3, n_new) and lg.shape == (n_new, 3, cfg.llm.vocab_size)
        differs = 0
        for b in range(3):
            for t in range(n_new):
                ctr = _dev([lens[b] - 1 + t], torch.int32)
                want = ops.sample(lg[t, b].contiguous(), kw["temperature"], top_k, top_p, seed + b, counter=ctr)
                assert int(ids[b, t]) == int(want), (top_k, b, t, int(ids[b, t]), int(want))
                differs += int(int(want) != int(lg[t, b].argmax()))
        assert differs > 0, "every draw equals its argmax: these inputs cannot tell a draw from a pick"
        lg_first = lg if lg_first is None else lg_first
        assert torch.equal(_bits(lg), _bits(lg_first))                 # teacher forcing: the logits do not depend on the pick
    # the pick is the only difference: the greedy batched step fed the same ids returns the same logits, bit for bit
    _, lg_greedy = llm._generate_batch(e, mask, n_new, -1, None, use_graph=False, forced_ids=forced, return_logits=True)
    assert not llm._bdecode.sampling and not getattr(llm._bdecode, "any_k", False)
    assert torch.equal(_bits(lg_greedy), _bits(lg_first))
    # the flag is read from generation_config as well
    from types import SimpleNamespace
    gc = SimpleNamespace(do_sample=True, temperature=0.9, top_k=0, top_p=0.9, batch_sample=True, any_top_k=True, max_new_tokens=3)
    out = llm.generate(inputs_embeds=e, attention_mask=mask, eos_token_id=-1, seed=seed, generation_config=gc)
    assert out.shape == (3, 3) and getattr(llm._bdecode, "any_k", False)


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_flagged_graph_equals_eager_and_one_graph_survives_every_kind_of_row(w4):
    cfg, model, e, mask, lens = _tiny(73, w4)
    llm = model.llm
    n_new = 10
    kw = dict(max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=0, top_p=0.9, batch_sample=True, any_top_k=True, attention_mask=mask)
    g = llm.generate(inputs_embeds=e, seed=77, use_graph=True, **kw)
    sess, graph = llm._bdecode, llm._bdecode.graph
    assert sess.any_k and graph is not None and g.shape == (3, n_new)
    assert torch.equal(llm.generate(inputs_embeds=e, seed=77, use_graph=False, **kw), g)
    assert llm._bdecode is sess and llm._bdecode.graph is graph
    # row 1 goes k = 30 -> 0 -> 500 -> greedy between replays of the ONE captured graph; rows 0 and 2 keep their parameters and their ids
    base = [(0.9, 0, 0.9, 77 + b) for b in range(3)]
    seen = []
    for row1 in ((1.2, 30, 0.95, 5), (1.2, 0, 0.95, 5), (1.2, 500, 0.95, 5), None):
        sampling = [base[0], row1, base[2]]
        got = llm._generate_batch(e, mask, n_new, -1, None, use_graph=True, sampling=sampling, any_top_k=True)
        assert llm._bdecode is sess and llm._bdecode.graph is graph, f"row 1 = {row1} re-captured the graph"
        assert torch.equal(got, llm._generate_batch(e, mask, n_new, -1, None, use_graph=False, sampling=sampling, any_top_k=True)), row1
        assert torch.equal(got[0], g[0]) and torch.equal(got[2], g[2])
        seen.append(tuple(got[1].tolist()))
    assert len(set(seen)) > 1
    # the greedy row of the flagged session is the greedy session's row
    greedy = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=-1)
    assert list(seen[3]) == greedy[1].tolist()
    # host-side validation: the flagged session takes every top_k >= 0, the unflagged one 1..64 as ever
    st = llm.batch_open(3, 256, 16, sampling=True, any_top_k=True)
    assert st.any_k and "any_top_k" in st.key
    for ok in ((0.5, 0, 0.9, 1), (0.5, 65, 0.9, 1), (0.5, 152064, 1.0, 1)):
        llm.batch_admit(st, 0, e[2, :5], sampling=ok)
    for bad in ((0.0, 0, 0.9, 1), (0.5, -1, 0.9, 1), (0.5, 0, 0.0, 1), (0.5, 0, 1.5, 1)):
        with pytest.raises(ValueError):
            llm.batch_admit(st, 0, e[2, :5], sampling=bad)
    st0 = llm.batch_open(3, 256, 16, sampling=True)
    assert st0 is not st and not getattr(st0, "any_k", False) and "any_top_k" not in st0.key
    with pytest.raises(ValueError, match="top_k in 1..64"):
        llm.batch_admit(st0, 0, e[2, :5], sampling=(0.5, 0, 0.9, 1))
    with pytest.raises(ValueError, match="sampling"):
        llm.batch_open(3, 256, 16, any_top_k=True)


def test_shared_prefix_return_sequences_draw_from_the_returned_logits():
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(75, False)
    llm = model.llm
    P, n_new, seed = 300, 6, 21
    ep = llm.embed_tokens(torch.randint(0, 900, (1, P), generator=torch.Generator().manual_seed(3)).cuda())
    for top_k, top_p in ((0, 0.9), (200, 1.0)):
        ids, lg = llm.generate(inputs_embeds=ep, max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=1.2, top_k=top_k, top_p=top_p, seed=seed,
                               batch_sample=True, any_top_k=True, num_return_sequences=3, return_logits=True)
        st = llm._bdecode
        assert st.shared_prefix and st.S == 256 and st.any_k and ids.shape == (3, n_new) and lg.shape[:2] == (n_new, 3)
        for j in range(3):
            for t in range(n_new):
                want = ops.sample(lg[t, j].contiguous(), 1.2, top_k, top_p, seed + j, counter=_dev([P - 1 + t], torch.int32))
                assert int(ids[j, t]) == int(want), (top_k, j, t)
        assert len({tuple(r) for r in ids.tolist()}) > 1
        g = llm.generate(inputs_embeds=ep, max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=1.2, top_k=top_k, top_p=top_p, seed=seed,
                         batch_sample=True, any_top_k=True, num_return_sequences=3)
        assert torch.equal(g, ids)                                     # the captured graph of the prefix session gives the eager ids
    with pytest.raises(ValueError, match="top_k in 1..64"):
        llm.generate(inputs_embeds=ep, max_new_tokens=2, do_sample=True, top_k=0, batch_sample=True, num_return_sequences=3)


def test_penalised_and_constrained_flagged_session_with_a_large_row():
    """A flagged session with penalties and automata: row 0 is a large row (top_k = 0) with penalties and an automaton, row 1 a plain greedy row.  Every
    token of row 0 is `ops.sample` on the processed row — the step's raw logits, penalised by the counts of what the row has generated
    (tests/penalty_ref.py, as test_gpu_penalties.py derives it), then masked by the automaton's state (as test_gpu_constrain.py derives it)."""
    from tests.test_gpu_constrain import EOS, TB
    from vila_amd import constrain as cn
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(77, False)
    llm, V, steps = model.llm, cfg.llm.vocab_size, 12
    a = cn.ConstraintCompiler(TB, EOS).regex(r"(yes|no|ab|abc|bc|[ ,01]|12|100)+")
    pen, smp = (1.3, 0.4, 0.2), (1.5, 0, 0.95, 31)
    st = llm.batch_open(3, 256, 16, sampling=True, penalties=True, constraints=True, any_top_k=True)
    assert st.any_k and st.pen is not None and st.con is not None
    llm.batch_release(st, [0, 1, 2])
    f0 = llm.batch_admit(st, 0, e[0, :20], sampling=smp, penalties=pen, constraint=a)
    f1 = llm.batch_admit(st, 1, e[1, :13])
    assert a.allowed(a.start)[f0]
    s, fed, row1 = a.step(a.start, f0), [f0], [f1]
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(st.stream):
        for t in range(steps):
            llm._batch_step(st)
            st.stream.synchronize()
            y = penalize_ref(st.logits[:1].cpu(), counts_of(fed, V), *pen)[0]
            y = torch.where(torch.from_numpy(a.allowed(s)), y, torch.full_like(y, float("-inf")))
            want = int(ops.sample(y.cuda(), smp[0], smp[1], smp[2], smp[3], counter=_dev([20 + t], torch.int32)))
            tok = int(st.token[0])
            assert tok == want, (t, tok, want)
            s = a.step(s, tok)
            fed.append(tok)
            assert int(st.token[1]) == int(st.logits[1].argmax())
            row1.append(int(st.token[1]))
    # the plain greedy neighbour is served as in a session without any flag
    st0 = llm.batch_open(3, 256, 16)
    llm.batch_release(st0, [0, 1, 2])
    llm.batch_admit(st0, 0, e[0, :20])
    g1 = llm.batch_admit(st0, 1, e[1, :13])
    llm.batch_run(st0, steps)
    assert [g1] + st0.out_ids[1, :steps].tolist() == row1


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_speculation_with_any_top_k_never_changes_the_ids(w4):
    """The reference run of test_gpu_spec_sample.py: the same sampled verify session drafting nothing (an empty candidate).  Lookup drafts over a
    history that holds the answer are accepted (at least one in the run) and change no id; a step whose every draft is accepted holds, row by row,
    the token `ops.sample` returns for that row's logits with counter S + j."""
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(79, w4)
    llm = model.llm
    g = torch.Generator().manual_seed(5)
    prompt = torch.randint(0, 900, (12,), generator=g).repeat(4)       # a repetitive prompt
    ep = llm.embed_tokens(prompt[None].cuda())
    S, n_new, empty = prompt.numel(), 20, torch.empty(0, dtype=torch.int64)

    def run(k_new, **kw):
        llm.spec_trace = []
        try:
            out = llm.generate(inputs_embeds=ep, max_new_tokens=k_new, eos_token_id=-1, prompt_lookup_num_tokens=4, spec_sample=True, any_top_k=True, **kw)
            return out[0].tolist(), list(llm.spec_trace)
        finally:
            llm.spec_trace = None

    for top_k, top_p in ((0, 0.9), (100, 1.0)):
        req = dict(do_sample=True, temperature=1.0, top_k=top_k, top_p=top_p, seed=1234)
        ids0, tr0 = run(n_new, draft_ids=empty, **req)
        st = llm._vdecode
        assert st.sampled and st.any_k and "any_top_k" in st.key and st.n == 5 and len(ids0) == n_new and tr0 == [0] * (n_new - 1)
        ids, tr = run(n_new, prompt_ids=torch.cat([prompt, torch.tensor(ids0)]), **req)
        print(f"top_k={top_k}: n_accept {tr}")
        assert ids == ids0, f"top_k={top_k}: lookup drafts changed the ids"
        assert sum(tr) >= 1, "no draft was accepted"
        assert llm._vdecode is st
        ids, tr = run(n_new, prompt_ids=prompt, **req)
        assert ids == ids0
        # one step of 5 rows, every draft accepted: the rows' draws are the solo sampler's
        _, tr = run(2, draft_ids=torch.tensor(ids0), **req)
        st = llm._vdecode                                              # (another max_out: a session of its own)
        assert tr == [4] and st.any_k and st.n == 5
        out = st.out_ids[:5].tolist()
        assert out == ids0[1:6]
        for j in range(5):
            want = int(ops.sample(st.logits[j], 1.0, top_k, top_p, 1234, counter=_dev([S + j], torch.int32)))
            assert out[j] == want, (top_k, j, out[j], want)
        # the first token is the solo sampled session's (same logits, same counter S - 1)
        assert llm.generate(inputs_embeds=ep, max_new_tokens=1, eos_token_id=-1, **req)[0].tolist() == ids0[:1]
    assert ids0 != llm.generate(inputs_embeds=ep, max_new_tokens=n_new, eos_token_id=-1)[0].tolist()
    for bad in (0, 100):                                               # without the flag the refusal is what it was
        with pytest.raises(ValueError, match="top_k in 1..64"):
            llm.generate(inputs_embeds=ep, max_new_tokens=4, prompt_lookup_num_tokens=4, spec_sample=True, do_sample=True, top_k=bad)


# ----------------------------------------------------------------------------------------------------------------------
# continuous batching
# ----------------------------------------------------------------------------------------------------------------------
def test_continuous_batching_admits_a_pure_top_p_request_beside_a_greedy_row():
    import time as _t
    from tests.test_serving_cpu import _Tok
    class Tok(_Tok):
        """Words in (the prompts); a reply spells its ids."""

        def decode(self, ids, skip_special_tokens=True):
            return " ".join(f"w{int(i)}" for i in ids)

    cfg, model, e, mask, lens = _tiny(81, False)
    tok = Tok()

    def serve(beside, flag=True):
        eng = serving.HipBatchEngine(model, tok, n_slots=4, max_ctx=256, max_new_tokens=64, eos_token_id=-1, sampling=True, **(dict(any_top_k=True) if flag else {}))
        cb = serving.ContinuousBatcher(eng, max_batch=4, chunk=2, batch_sampled=True, **(dict(any_top_k=True) if flag else {}))
        try:
            fa = None
            if beside:
                fa = cb.submit("describe the image in many words", 48)  # long, greedy
                while not any(ev[0] == "run" for ev in cb.events):
                    _t.sleep(0.001)
            fb = cb.submit("what is this ?", 8, temperature=0.9, top_p=0.9, top_k=0, seed=5)
            tb = fb.result(timeout=120)
            return (None if fa is None else fa.result(timeout=120)), tb, list(cb.events), cb
        finally:
            cb.close()

    ta, tb, ev, cb = serve(True)
    assert cb.any_top_k and model.llm._bdecode.any_k
    admits = [x for x in ev if x[0] == "admit"]
    assert len(admits) == 2 and admits[1][2] > 0 and admits[1][3] == 1, admits      # the request joined while the greedy row ran
    assert not any(x[0] == "solo" for x in ev)
    assert isinstance(ta, str) and ta and isinstance(tb, str)
    _, tb1, ev1, _ = serve(False)                                       # the same request alone: a one-row flagged session
    assert not any(x[0] == "solo" for x in ev1) and tb1 == tb
    _, _, ev0, cb0 = serve(True, flag=False)                            # without the flag it runs solo, as ever
    assert not cb0.any_top_k and any(x[0] == "solo" for x in ev0)

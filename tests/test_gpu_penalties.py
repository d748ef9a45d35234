"""Repetition, presence and frequency penalties in the device pick (vila_logits_penalize_f32, vila_llm_decode_step[_batch]_penalized,
generate(repetition_penalty=, presence_penalty=, frequency_penalty=), batch_open(penalties=True)).

The processed logits are one rounded fp32 operation per step, so everything here is compared BIT FOR BIT with the torch expression on the CPU
(tests/penalty_ref.py, which tests/test_penalties_cpu.py pins to transformers' RepetitionPenaltyLogitsProcessor): the operator's output, its
(max, first index) pairs, and every id a penalised step returns — recomputed on the CPU from the raw logits the step returned and the ids fed so far."""
import pytest
import torch

from tests.penalty_ref import counts_of, first_argmax, from_u16_bits, penalize_ref, u16_bits
from vila_amd import configs

pytestmark = pytest.mark.gpu

PARAMS = [(1.05, 0.0, 0.0), (1.3, 0.5, 0.25), (0.02, 0.0, 0.0), (1.0, -3.0, -1e4), (1.0, 0.0, 0.0)]


def _dev(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _operator_inputs(n, V, seed):
    """Random logits with planted cases, counts drawn from {0, 1, 2, 65535}."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, V, generator=g) * 3
    c = torch.tensor([0, 1, 2, 65535])[torch.randint(0, 4, (n, V), generator=g)]
    for r in range(n):
        z = 7 + 11 * r                                                 # exact zeros and -0.0, with and without a count
        x[r, z], x[r, z + 1], x[r, z + 2], x[r, z + 3] = 0.0, -0.0, 0.0, -0.0
        c[r, z], c[r, z + 1], c[r, z + 2], c[r, z + 3] = 0, 0, 2, 65535
        # two planted ties in the processed values: neighbours (one thread's vector) and half a row apart (another block), at the row's largest
        # unpenalised value (count 0: y = x whatever the parameters) ...
        d = 200 + 4 * r + 1
        for i in (d, d + 1, d + V // 2):
            x[r, i], c[r, i] = 45.0, 0
        # ... and at equal logits with equal counts, which every parameter set maps to equal values
        a = 120 + 3 * r
        for i in (a, a + 2, a + V // 3):
            x[r, i], c[r, i] = 40.0, 65535
    return x, c


@pytest.mark.parametrize("V", [1001, 152064])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_operator_is_bit_equal_to_the_torch_expression(n, V):
    from vila_amd import ops
    x, c = _operator_inputs(n, V, 100 * n + V)
    mixed = [PARAMS[r % len(PARAMS)] for r in range(n)]
    for name, rows in [(str(p), [p] * n) for p in PARAMS] + [("mixed", mixed)]:
        rep, pres, freq = ([p[k] for p in rows] for k in range(3))
        want = penalize_ref(x, c, rep, pres, freq)
        # tight rows; rows vocab + 37 apart (unaligned: the scalar path); rows padded to the next multiple of 4 and 4 more (aligned rows whose end
        # is no whole vector where the vocabulary is no multiple of 4).  1e9 beyond the vocabulary: nothing there may be read
        for tight, pad in ((True, 0), (False, 37), (False, (4 - V % 4) % 4 + 4)):
            if tight:
                lg, cnt = x.cuda(), u16_bits(c).cuda()
            else:
                wide = torch.full((n, V + pad), 1e9)
                wide[:, :V] = x
                lg = wide.cuda()[:, :V]
                cw = torch.full((n, V + pad), 65535)
                cw[:, :V] = c
                cnt = u16_bits(cw).cuda()[:, :V]
            before = cnt.clone()
            y, pv, pi = ops.penalize(lg, cnt, _dev(rep, torch.float32), _dev(pres, torch.float32), _dev(freq, torch.float32), return_pick=True)
            assert torch.equal(_bits(y), _bits(want)), (name, tight, int((_bits(y) != _bits(want)).sum()))
            assert torch.equal(cnt, before), "no token: no bump"
            if rows[0] == (1.0, 0.0, 0.0) and name != "mixed":
                assert torch.equal(_bits(y), _bits(x)), "neutral parameters must return the input bits"
            pv, pi = pv.cpu(), pi.cpu()
            for r in range(n):
                best = pv[r].max()
                got = int(pi[r][pv[r] == best].min())                  # the merge of the pairs: largest value, then the lower index
                assert got == first_argmax(want[r]), (name, tight, r, got, first_argmax(want[r]))
                assert float(best) == float(want[r].max())
                ok = pi[r] < V                                         # (an empty slice leaves an index beyond every real one)
                assert bool((want[r][pi[r][ok].long()] == pv[r][ok]).all()), "a pair's value is the processed logit at its index"
    # the planted ties decide a pick: with (1.05, 0, 0) the row's maximum is the count-0 tie at 45, whose first index is the expected one
    want = penalize_ref(x, c, 1.05, 0.0, 0.0)
    assert all(first_argmax(want[r]) == 200 + 4 * r + 1 and float(want[r].max()) == 45.0 for r in range(n))


@pytest.mark.parametrize("V", [1001, 152064])
def test_bump_counts_the_consumed_token_once_and_saturates(V):
    from vila_amd import ops
    n = 6
    x, c = _operator_inputs(n, V, 5 + V)
    tok = [17, 17, V - 1, 0, -1, V]                                    # rows 0 and 1 consume the same id; -1 and V bump nothing
    c[0, 17], c[1, 17], c[2, V - 1], c[3, 0] = 0, 2, 65535, 65534
    want_c = c.clone()
    want_c[0, 17], want_c[1, 17], want_c[3, 0] = 1, 3, 65535           # 65535 stays 65535
    rep, pres, freq = [1.3] * n, [0.5] * n, [0.25] * n
    for tight in (True, False):
        if tight:
            lg, cnt = x.cuda(), u16_bits(c).cuda()
        else:
            lg = torch.cat([x, torch.full((n, 37), 1e9)], 1).cuda()[:, :V]
            cnt = u16_bits(torch.cat([c, torch.full((n, 37), 7)], 1)).cuda()
            whole, cnt = cnt, cnt[:, :V]
        y = ops.penalize(lg, cnt, _dev(rep, torch.float32), _dev(pres, torch.float32), _dev(freq, torch.float32), token=_dev(tok, torch.int64))
        assert torch.equal(from_u16_bits(cnt), want_c), "exactly one count per row rises by one, nothing else changes"
        if not tight:
            assert bool((from_u16_bits(whole[:, V:]) == 7).all()), "nothing beyond the vocabulary is written"
        # the owner of the index bumps before it reads: the processed row uses the new count
        assert torch.equal(_bits(y), _bits(penalize_ref(x, want_c, rep, pres, freq)))


# ----------------------------------------------------------------------------------------------------------------------
# the steps, on configs.tiny
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


N_NEW = 9
SAMPLING = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95)


def _expected(lg_row, fed, pen, V, sampling=None, seed=0, counter=0):
    """The pick of one step on the CPU: lg_row = the raw logits the step returned, fed = the ids it and the steps before it consumed."""
    from vila_amd import ops
    y = penalize_ref(lg_row[None].cpu(), counts_of(fed, V), *pen)[0]
    if sampling is None:
        return first_argmax(y)
    return int(ops.sample(y.cuda(), sampling["temperature"], sampling["top_k"], sampling["top_p"], seed, counter=_dev([counter], torch.int32)))


def _check_rows(ids, lg, forced, lens, pen, V, sampling, seed):
    """ids [B, n], lg [n, B, V], forced [B, n]: every returned id is the CPU's pick.  Step 0 is the prefill's pick (nothing generated yet: never
    penalised); step t >= 1 consumed forced[:, t - 1] at position len - 1 + t and has counted forced[:, :t]."""
    differs = 0
    for b in range(ids.shape[0]):
        for t in range(ids.shape[1]):
            fed = forced[b, :t].tolist()
            want = _expected(lg[t, b], fed, pen, V, sampling, seed + b, lens[b] - 1 + t)
            assert int(ids[b, t]) == want, (b, t, int(ids[b, t]), want)
            differs += int(int(ids[b, t]) != first_argmax(lg[t, b].cpu()))
    return differs


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_batched_step_picks_from_the_penalised_logits(w4, sampled):
    cfg, model, e, mask, lens = _tiny(41, w4)
    llm, V, seed = model.llm, cfg.llm.vocab_size, 4242
    forced = torch.randint(0, 40, (3, N_NEW), generator=torch.Generator().manual_seed(9))     # a small alphabet: ids repeat within a row
    kw = dict(inputs_embeds=e, attention_mask=mask, max_new_tokens=N_NEW, eos_token_id=-1)
    if sampled:
        kw.update(SAMPLING, seed=seed, batch_sample=True)
    sampling = SAMPLING if sampled else None
    _, lg_plain = llm._generate_batch(e, mask, N_NEW, -1, None, use_graph=False, forced_ids=forced, return_logits=True)
    for pen in ((1.3, 0.5, 0.25), (1.0, 0.0, -1e4)):
        ids, lg = llm.generate(**kw, return_logits=True, forced_ids=forced, use_graph=False, repetition_penalty=pen[0], presence_penalty=pen[1],
                               frequency_penalty=pen[2])
        st = llm._bdecode
        assert st is not None and st.pen is not None and st.sampling == sampled, "the penalised batch did not take the penalised batched step"
        assert ids.shape == (3, N_NEW) and lg.shape == (N_NEW, 3, V)
        differs = _check_rows(ids.cpu(), lg, forced, lens, pen, V, sampling, seed)
        # st->logits stays the raw model logits: the same bits as the unpenalised greedy step fed the same ids
        assert torch.equal(_bits(lg), _bits(lg_plain))
        if pen[2] == -1e4:                                             # a reward of 1e4 per repeat: every later pick lies in the row's history
            for b in range(3):
                for t in range(1, N_NEW):
                    assert int(ids[b, t]) in forced[b, :t].tolist(), (b, t)
            assert differs >= 1, "no pick differed from the raw argmax"
    # graph = eager, and the free-running ids are the CPU's picks when they are fed back
    pen = (1.3, 0.5, 0.25)
    pk = dict(repetition_penalty=pen[0], presence_penalty=pen[1], frequency_penalty=pen[2])
    g = llm.generate(**kw, use_graph=True, **pk)
    assert llm._bdecode.pen is not None and llm._bdecode.graph is not None
    assert torch.equal(g, llm.generate(**kw, use_graph=False, **pk))
    ids, lg = llm.generate(**kw, return_logits=True, forced_ids=g, use_graph=False, **pk)
    assert torch.equal(ids, g)
    _check_rows(ids.cpu(), lg, g.cpu(), lens, pen, V, sampling, seed)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_solo_step_picks_from_the_penalised_logits(w4, sampled):
    cfg, model, e, mask, lens = _tiny(43, w4)
    llm, V, seed = model.llm, cfg.llm.vocab_size, 77
    forced = torch.randint(0, 40, (N_NEW,), generator=torch.Generator().manual_seed(10))
    kw = dict(inputs_embeds=e[:1], max_new_tokens=N_NEW, eos_token_id=-1)
    if sampled:
        kw.update(SAMPLING, seed=seed)
    sampling = SAMPLING if sampled else None
    _, lg_plain = llm.generate(**kw, return_logits=True, forced_ids=forced)
    assert llm._decode.pen is None
    for pen in ((1.3, 0.5, 0.25), (1.0, 0.0, -1e4)):
        ids, lg = llm.generate(**kw, return_logits=True, forced_ids=forced, repetition_penalty=pen[0], presence_penalty=pen[1], frequency_penalty=pen[2])
        assert llm._decode.pen is not None and (llm._decode.sampling is not None) == sampled
        assert ids.shape == (1, N_NEW) and lg.shape == (N_NEW, V)
        differs = _check_rows(ids.cpu(), lg[:, None], forced[None], lens[:1], pen, V, sampling, seed)
        assert torch.equal(_bits(lg), _bits(lg_plain))
        if pen[2] == -1e4:
            assert all(int(ids[0, t]) in forced[:t].tolist() for t in range(1, N_NEW))
            assert differs >= 1
    pen = (1.3, 0.5, 0.25)
    pk = dict(repetition_penalty=pen[0], presence_penalty=pen[1], frequency_penalty=pen[2])
    g = llm.generate(**kw, use_graph=True, **pk)
    assert llm._decode.pen is not None and llm._decode.graph is not None
    assert torch.equal(g, llm.generate(**kw, use_graph=False, **pk))
    ids, lg = llm.generate(**kw, return_logits=True, forced_ids=g[0], **pk)
    assert torch.equal(ids, g)
    _check_rows(ids.cpu(), lg[:, None], g.cpu(), lens[:1], pen, V, sampling, seed)


def test_neutral_parameters_on_a_penalised_session_give_the_plain_ids():
    cfg, model, e, mask, lens = _tiny(45, False)
    llm, n_new, neutral = model.llm, 12, (1.0, 0.0, 0.0)
    for graph in (True, False):
        # solo, greedy and sampled
        plain = llm.generate(inputs_embeds=e[:1], max_new_tokens=n_new, eos_token_id=-1, use_graph=graph)
        assert llm._decode.pen is None
        pen = llm._generate_solo(e[:1], None, n_new, -1, None, graph, False, None, None, None, penalties=neutral)
        assert llm._decode.pen is not None and torch.equal(pen, plain)
        samp = (0.9, 30, 0.95, 5)
        plain = llm._generate_solo(e[:1], None, n_new, -1, samp, graph, False, None, None, None)
        pen = llm._generate_solo(e[:1], None, n_new, -1, samp, graph, False, None, None, None, penalties=neutral)
        assert llm._decode.pen is not None and torch.equal(pen, plain)
        # batched, greedy and sampled rows
        plain = llm._generate_batch(e, mask, n_new, -1, None, use_graph=graph)
        assert llm._bdecode.pen is None
        pen = llm._generate_batch(e, mask, n_new, -1, None, use_graph=graph, penalties=neutral)
        assert llm._bdecode.pen is not None and torch.equal(pen, plain)
        rows = [(0.9, 30, 0.95, 5), None, (1.4, 64, 1.0, 6)]
        plain = llm._generate_batch(e, mask, n_new, -1, None, use_graph=graph, sampling=rows)
        pen = llm._generate_batch(e, mask, n_new, -1, None, use_graph=graph, sampling=rows, penalties=neutral)
        assert llm._bdecode.pen is not None and llm._bdecode.sampling and torch.equal(pen, plain)
    # one shared-prefix session: three samples of one prompt of 300 positions
    ep = llm.embed_tokens(torch.randint(0, 900, (1, 300), generator=torch.Generator().manual_seed(3)).cuda())
    kw = dict(inputs_embeds=ep, max_new_tokens=6, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=21, batch_sample=True,
              num_return_sequences=3)
    plain = llm.generate(**kw)
    assert llm._bdecode.shared_prefix and llm._bdecode.S == 256 and llm._bdecode.pen is None
    rows = [llm._check_batch_sampling((0.9, 30, 0.95, 21 + j), "test") for j in range(3)]
    pen = llm._generate_shared(ep, 3, 6, -1, None, True, False, rows, penalties=neutral)
    assert llm._bdecode.shared_prefix and llm._bdecode.S == 256 and llm._bdecode.pen is not None
    assert plain.shape == (3, 6) and torch.equal(pen, plain)
    # ... and a non-neutral request through the public call runs on such a session and changes the ids' distribution only through the pick
    out = llm.generate(**kw, frequency_penalty=-1e4)
    assert llm._bdecode.pen is not None and out.shape == (3, 6)
    for r in out.tolist():
        assert all(r[t] in r[:t] for t in range(2, 6)), r              # (the first generated token is counted from the second step on)


def test_one_captured_graph_serves_a_change_of_penalties():
    cfg, model, e, mask, lens = _tiny(47, False)
    llm, n_new = model.llm, 12
    kw = dict(max_new_tokens=n_new, eos_token_id=-1)
    a = llm.generate(inputs_embeds=e[:1], repetition_penalty=1.3, **kw)
    sess, graph = llm._decode, llm._decode.graph
    assert sess.pen is not None and graph is not None
    b = llm.generate(inputs_embeds=e[:1], repetition_penalty=1.0, presence_penalty=0.7, frequency_penalty=-1e4, **kw)
    assert llm._decode is sess and llm._decode.graph is graph, "other penalty values re-captured the graph"
    # the second call's counts started from zero: its ids are those of an eager run
    assert torch.equal(b, llm.generate(inputs_embeds=e[:1], repetition_penalty=1.0, presence_penalty=0.7, frequency_penalty=-1e4, use_graph=False, **kw))
    assert torch.equal(a, llm.generate(inputs_embeds=e[:1], repetition_penalty=1.3, **kw)) and not torch.equal(a, b)
    assert llm._decode is sess and llm._decode.graph is graph
    # the batched session likewise
    a = llm.generate(inputs_embeds=e, attention_mask=mask, repetition_penalty=1.3, **kw)
    sess, graph = llm._bdecode, llm._bdecode.graph
    assert sess.pen is not None and graph is not None
    b = llm.generate(inputs_embeds=e, attention_mask=mask, frequency_penalty=-1e4, **kw)
    assert llm._bdecode is sess and llm._bdecode.graph is graph
    assert torch.equal(b, llm.generate(inputs_embeds=e, attention_mask=mask, frequency_penalty=-1e4, use_graph=False, **kw))
    assert not torch.equal(a, b)
    # neutral values leave the penalised sessions alone and take the plain ones
    llm.generate(inputs_embeds=e, attention_mask=mask, repetition_penalty=1.0, **kw)
    assert llm._bdecode is not sess and llm._bdecode.pen is None


def test_continuous_batching_a_penalised_row_beside_a_plain_one():
    cfg, model, e, mask, lens = _tiny(49, False)
    llm, steps = model.llm, 10

    def run(row1):
        """Row 0 plain and live; after 3 steps row 1 joins with `row1` penalties (None = plain); -> (row 0's ids, row 1's ids)."""
        st = llm.batch_open(3, 256, 16, penalties=True)
        llm.batch_release(st, [0, 1, 2])
        f0 = llm.batch_admit(st, 0, e[0, :20])
        llm.batch_run(st, 3)
        f1 = llm.batch_admit(st, 1, e[1, :13], penalties=row1)
        assert int(from_u16_bits(st.counts[1]).sum()) == 0, "an admitted row starts from zero counts"
        llm.batch_run(st, steps)
        return st, [f0] + st.out_ids[0, :steps + 3].tolist(), [f1] + st.out_ids[1, :steps].tolist()

    st, a0, a1 = run((1.0, 0.0, -1e4))
    graph = st.graph
    assert st.pen is not None and "penalties" in st.key and graph is not None
    assert st.p_freq.tolist()[:2] == [0.0, -1e4] and st.p_rep.tolist() == [1.0, 1.0, 1.0]
    assert all(a1[t] in a1[:t] for t in range(2, steps + 1)), a1       # the penalty acted on row 1
    assert int(from_u16_bits(st.counts[1]).sum()) == steps             # one count per consumed token
    st2, b0, b1 = run(None)
    assert st2 is st and st.graph is graph
    assert a0 == b0, "a penalised neighbour changed the plain row's ids"
    assert a1 != b1
    # the slot is re-used: the same request there again starts from zero counts and repeats its ids
    _, c0, c1 = run((1.0, 0.0, -1e4))
    assert c0 == a0 and c1 == a1
    # a plain session gives row 0 the same ids, and refuses a penalised row
    stp = llm.batch_open(3, 256, 16)
    assert stp is not st and stp.pen is None
    llm.batch_release(stp, [0, 1, 2])
    f0 = llm.batch_admit(stp, 0, e[0, :20])
    llm.batch_run(stp, steps + 3)
    assert [f0] + stp.out_ids[0, :steps + 3].tolist() == a0
    with pytest.raises(ValueError, match="penalties=True"):
        llm.batch_admit(stp, 1, e[1, :13], penalties=(1.1, 0.0, 0.0))
    with pytest.raises(ValueError, match="strictly positive"):
        llm.batch_admit(llm.batch_open(3, 256, 16, penalties=True), 1, e[1, :13], penalties=(0.0, 0.0, 0.0))

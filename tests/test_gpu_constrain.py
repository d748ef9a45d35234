"""Structured output on the device (vila_logits_constrain_f32, vila_llm_decode_step[_batch]_constrained, generate(constraint=),
batch_open(constraints=True)).

Everything is exact: a processed logit is the input's bits or -inf, states, ids and pairs are integers.  The operator is compared bit for bit with
tests/constrain_ref.py; every id a constrained step returns is recomputed on the host from the raw logits the step returned (`return_logits`) and
`Automaton.allowed` — the same bits, since the launches in front of the pick are the plain step's."""
import numpy as np
import pytest
import torch

from tests.constrain_ref import EOS_IDS, constrain_ref, masked_first_argmax, merge_pairs, pairs_ref, synthetic_vocab
from vila_amd import configs
from vila_amd import constrain as cn

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
MAX_C = 4096


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _dev(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device="cuda")


def _u16(a):
    """uint16 values -> the int16 tensor with the same bits."""
    return torch.from_numpy(np.asarray(a).astype(np.uint16).view(np.int16).copy())


def _framed(vals: torch.Tensor, pad: int, offset: int, fill):
    """vals [n, V] as a view of a 1-D buffer: a guard row in front and behind, rows V + pad apart, the first `offset` elements in. -> (view, buffer, mask
    of the view inside the buffer)."""
    n, V = vals.shape
    ld = V + pad
    buf = torch.full(((n + 2) * ld + offset,), fill, dtype=vals.dtype, device="cuda")
    view = buf[ld + offset:ld + offset + n * ld].view(n, ld)[:, :V]
    view.copy_(vals)
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    inside[ld + offset:ld + offset + n * ld].view(n, ld)[:, :V] = True
    return view, buf, inside


def _rows(n, V, seed):
    """n rows with different automata: unconstrained rows, C = 1, C = the cap, small C; state 2 of every table allows ONLY id V - 1, state 3 nothing."""
    rng = np.random.default_rng(seed)
    S = 5
    specs = []
    for r in range(n):
        kind = r % 4 if n > 1 else 3
        C = {0: 7, 1: 1, 2: MAX_C, 3: 11}[kind]
        cls = rng.integers(0, max(C - 1, 1), size=V)                # class C - 1 is kept for id V - 1 alone (C > 1)
        cls[V - 1] = C - 1
        nxt = np.where(rng.random((S, C)) < 0.5, rng.integers(0, S, size=(S, C)), -1)
        if C > 1:
            nxt[2, :] = -1
            nxt[2, C - 1] = 4
        nxt[3, :] = -1
        state = -1 if (kind == 0 and n > 1) else int(rng.integers(0, S))
        specs.append(dict(C=C, cls=cls, nxt=nxt.astype(np.int16), state=state))
    if n >= 3:
        specs[1]["state"], specs[2]["state"] = 3, 2               # all-disallowed (C = 1) and only-the-last-id (C = cap)
    else:
        specs[0]["state"] = 2
    return specs, S


@pytest.mark.parametrize("V", [1003, 1000, 8])
@pytest.mark.parametrize("n", [1, 3, 16])
def test_operator_is_bit_equal_to_the_reference(n, V):
    from vila_amd import ops
    specs, S = _rows(n, V, 7 * n + V)
    g = torch.Generator().manual_seed(n + V)
    x = torch.randn(n, V, generator=g) * 3
    x[:, V // 2] = x[:, 0] = 9.0                                      # a tie across slices: the first index wins
    ld_next = S * MAX_C + 3
    nxt = np.full((n, ld_next), 12345, dtype=np.int16)                # (beyond a row's own table: never read)
    for r, sp in enumerate(specs):
        nxt[r, :S * sp["C"]] = sp["nxt"].reshape(-1)
    cls = np.stack([sp["cls"] for sp in specs])
    ncl = [sp["C"] for sp in specs]
    state0 = [sp["state"] for sp in specs]
    # tokens: allowed, disallowed, out of range on both sides, the last id
    toks = []
    for r, sp in enumerate(specs):
        s = sp["state"]
        ok = np.flatnonzero(sp["nxt"][max(s, 0)][sp["cls"]] >= 0)
        bad = np.flatnonzero(sp["nxt"][max(s, 0)][sp["cls"]] < 0)
        toks.append([int(ok[0]) if ok.size else V - 1, int(bad[0]) if bad.size else 0, -1, V, V - 1][r % 5])
    n_slices = None
    for layout, (pad, off) in dict(aligned=((4 - V % 4) % 4 + 4, 0), offset=(37, 1), tight=(0, 0)).items():
        for token in (None, toks):
            for alias in (False, True):
                lg, lbuf, lin = _framed(x, pad, off, float("nan"))
                if layout == "aligned":
                    assert lg.data_ptr() % 16 == 0 and (V + pad) % 4 == 0, "the aligned layout must reach the vector path"
                cl, cbuf, cin = _framed(_u16(cls), pad, off * 3 if off else 0, -1)
                st = _dev(state0, torch.int32)
                tk = None if token is None else _dev(token, torch.int64)
                if alias:
                    out, obuf, oin = lg, lbuf, lin
                else:
                    out, obuf, oin = _framed(torch.zeros(n, V), pad, off, 0.0)
                    obuf.view(torch.int32).masked_fill_(~oin, GUARD)
                want_y, want_s = constrain_ref(x.numpy(), state0, cls, nxt, ncl, token)
                runs = []
                for _ in range(2):
                    if alias:
                        lg.copy_(x)
                    st.copy_(_dev(state0, torch.int32))
                    y, pv, pi = ops.logits_constrain(lg, st, cl, torch.from_numpy(nxt).cuda(), _dev(ncl, torch.int32), token=tk, return_pick=True, out=out)
                    assert y.data_ptr() == out.data_ptr()
                    runs.append((_bits(y), st.cpu().clone(), _bits(pv), pi.cpu().clone()))
                what = (layout, token is not None, alias)
                assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), ("two runs differ", what)
                yb, sb, pvb, pib = runs[0]
                assert torch.equal(yb, _bits(torch.from_numpy(want_y))), (what, int((yb != _bits(torch.from_numpy(want_y))).sum()))
                assert sb.tolist() == want_s.tolist(), (what, sb.tolist(), want_s.tolist())
                n_slices = pib.shape[1]
                wv, wi = pairs_ref(want_y, n_slices)
                assert torch.equal(pvb, _bits(torch.from_numpy(wv))) and pib.tolist() == wi.tolist(), what
                # guard words: nothing outside the views was written (NaN padding of the logits, -1 of the classes, the pattern of the output)
                if not alias:
                    assert bool((obuf.view(torch.int32)[~oin] == GUARD).all()), (what, "the output frame was written")
                    assert bool(torch.isnan(lbuf[~lin]).all()) and torch.equal(_bits(lg), _bits(x)), (what, "the logits were written")
                else:
                    assert bool(torch.isnan(lbuf[~lin]).all()), (what, "the aliased frame was written")
                assert bool((cbuf[~cin] == -1).all())
                for r, sp in enumerate(specs):
                    v, i = merge_pairs(wv[r], wi[r])
                    if want_s[r] < 0:
                        assert np.array_equal(want_y[r].view(np.int32), x[r].numpy().view(np.int32)), "an unconstrained row keeps its bits"
                    elif want_s[r] == 3:
                        assert v == -np.inf and i == 0, "an all-disallowed state merges to index 0"
                    elif want_s[r] == 2 and sp["C"] > 1:
                        assert i == V - 1 and np.isinf(want_y[r][:V - 1]).all(), "only the last id is allowed"
    assert n_slices == 32


def test_operator_refuses_bad_arguments():
    from vila_amd import _lib, ops
    import ctypes as C
    lib = _lib.load()
    x = torch.zeros(2, 8, device="cuda")
    st, cl, nx, nc = _dev([0, 0], torch.int32), torch.zeros(2, 8, dtype=torch.int16, device="cuda"), torch.zeros(2, 4, dtype=torch.int16, device="cuda"), _dev([1, 1], torch.int32)
    pv = torch.zeros(2, 32, device="cuda")

    def call(logits=x.data_ptr(), ld=8, n=2, V=8, con=None, out=x.data_ptr(), ld_out=8, v=None, i=None, ld_cls=8, state=st.data_ptr()):
        c = _lib.VilaConstraints(state, cl.data_ptr(), ld_cls, nx.data_ptr(), 4, nc.data_ptr())
        return lib.vila_logits_constrain_f32(logits, ld, n, V, C.byref(c) if con is None else con, None, out, ld_out, v, i, ops._stream())

    assert call() == 0
    for kw in (dict(logits=None), dict(out=None), dict(ld=7), dict(ld_out=7), dict(ld_cls=7), dict(n=0), dict(n=65536), dict(state=None), dict(v=pv.data_ptr()),
               dict(con=C.POINTER(_lib.VilaConstraints)())):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.logits_constrain(x, st, cl[:, :7], nx, nc)


# ----------------------------------------------------------------------------------------------------------------------
# the steps, on configs.tiny (vocab 1000) with the synthetic vocabulary
# ----------------------------------------------------------------------------------------------------------------------
EOS = list(EOS_IDS)
TB = synthetic_vocab()
CHOICES = ["yes", "no", "no!", "abc", "true"]
SCHEMA = {"type": "object", "properties": {"name": {"type": "string", "maxLength": 3}, "ok": {"type": "boolean"},
                                           "tags": {"type": "array", "items": {"enum": ["red", "green", 12]}, "maxItems": 2}}}


@pytest.fixture(scope="module")
def automata():
    comp = cn.ConstraintCompiler(TB, EOS)
    return dict(choice=comp.choice(CHOICES), schema=comp.json_schema(SCHEMA), schema2=comp.json_schema(SCHEMA, indent=2),
                loop=comp.regex(r"(yes|no|ab|abc|bc|[ ,01]|12|100)+"), dfa=dict(choice=cn.byte_dfa(cn.choice(CHOICES)), schema=cn.byte_dfa(cn.json_schema(SCHEMA)),
                                                                                schema2=cn.byte_dfa(cn.json_schema(SCHEMA, indent=2))))


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


def _text(ids):
    """The bytes of a row up to its first EOS, and whether it reached one."""
    out = b""
    for t in ids:
        if int(t) in EOS_IDS:
            return out, True
        out += TB[int(t)]
    return out, False


def _check_greedy(ids_row, lg_rows, a):
    """Every id is the first maximum of the step's raw logits under the automaton's mask, the state advanced by the ids before it."""
    s = a.start
    for t, tok in enumerate(ids_row):
        want = masked_first_argmax(lg_rows[t].cpu().numpy(), a.allowed(s))
        assert int(tok) == want, (t, int(tok), want)
        s = a.step(s, want)
    return s


N_NEW = 128        # the longest member of the schemas below, spelt byte by byte, and its EOS


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_solo_greedy_ids_are_the_masked_argmax_of_the_raw_logits(w4, automata):
    cfg, model, e, mask, lens = _tiny(51, w4)
    llm = model.llm
    kw = dict(inputs_embeds=e[:1], max_new_tokens=N_NEW, eos_token_id=EOS)
    _, lg_plain = llm.generate(**kw, return_logits=True)
    assert llm._decode.con is None
    sess = None
    for name in ("choice", "schema", "schema2"):
        a = automata[name]
        ids, lg = llm.generate(**kw, constraint=a, return_logits=True)
        assert llm._decode.con is not None and "constraints" in llm._decode.key
        assert torch.equal(_bits(lg[0]), _bits(lg_plain[0])), "return_logits stays raw"
        _check_greedy(ids[0].tolist(), lg, a)
        text, done = _text(ids[0].tolist())
        assert done and cn.dfa_accepts(automata["dfa"][name], text), (name, text)
        g = llm.generate(**kw, constraint=a)                          # the captured graph gives the eager ids
        assert llm._decode.graph is not None and torch.equal(g, ids) and torch.equal(g, llm.generate(**kw, constraint=a, use_graph=False))
        sess = sess or (llm._decode, llm._decode.graph)
        assert (llm._decode, llm._decode.graph) == sess, "another automaton re-captured the graph"
    for bad in (dict(prompt_lookup_num_tokens=3), dict(forced_ids=torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(ValueError, match="constraint is not served"):
            llm.generate(**kw, constraint=automata["choice"], **bad)


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_batched_greedy_ids_are_the_masked_argmax_of_the_raw_logits(w4, automata):
    cfg, model, e, mask, lens = _tiny(53, w4)
    llm = model.llm
    kw = dict(inputs_embeds=e, attention_mask=mask, max_new_tokens=N_NEW, eos_token_id=EOS)
    for name in ("choice", "schema"):
        a = automata[name]
        ids, lg = llm.generate(**kw, constraint=a, return_logits=True)
        st = llm._bdecode
        assert st is not None and st.con is not None and ids.shape == (3, N_NEW) and lg.shape[:2] == (N_NEW, 3)
        for b in range(3):
            s = _check_greedy(ids[b].tolist(), lg[:, b], a)
            text, done = _text(ids[b].tolist())
            assert done and s == a.n_states - 1 and cn.dfa_accepts(automata["dfa"][name], text), (name, b, text)
        g = llm.generate(**kw, constraint=a)
        assert llm._bdecode.graph is not None and torch.equal(g, llm.generate(**kw, constraint=a, use_graph=False))
        for b in range(3):
            assert _text(g[b].tolist())[0] == _text(ids[b].tolist())[0]


SAMPLING = dict(do_sample=True, temperature=1.5, top_k=30, top_p=0.95)


@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_sampled_rows_draw_from_the_processed_row_and_never_leave_the_language(w4, automata):
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(55, w4)
    llm, a, n_new = model.llm, automata["loop"], 100
    few = 0
    for seed in (11, 12):
        ids, lg = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=-1, constraint=a, return_logits=True,
                               batch_sample=True, seed=seed, **SAMPLING)
        assert llm._bdecode.con is not None and llm._bdecode.sampling
        for b in range(3):
            s = a.start
            for t in range(n_new):
                ok = a.allowed(s)
                tok = int(ids[b, t])
                assert ok[tok], (seed, b, t, tok)
                few += int(ok.sum() < SAMPLING["top_k"])
                if t % 7 == 0 or ok.sum() < SAMPLING["top_k"] and t < 40:     # the draw itself, on a sample of the steps
                    y = torch.where(torch.from_numpy(ok).cuda(), lg[t, b], torch.full_like(lg[t, b], float("-inf")))
                    want = int(ops.sample(y, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], seed + b, counter=_dev([lens[b] - 1 + t], torch.int32)))
                    assert tok == want, (seed, b, t, tok, want)
                s = a.step(s, tok)
    assert few > 0, "no state with fewer allowed tokens than top_k was visited"
    # solo: a choice state has one to three allowed tokens, far fewer than top_k
    c = automata["choice"]
    for seed in range(5):
        ids, lg = llm.generate(inputs_embeds=e[:1], max_new_tokens=8, eos_token_id=EOS, constraint=c, return_logits=True, seed=seed, **SAMPLING)
        s = c.start
        for t, tok in enumerate(ids[0].tolist()):
            ok = c.allowed(s)
            y = torch.where(torch.from_numpy(ok).cuda(), lg[t], torch.full_like(lg[t], float("-inf")))
            assert ok[tok] and tok == int(ops.sample(y, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], seed, counter=_dev([19 + t], torch.int32)))
            s = c.step(s, tok)
        text, done = _text(ids[0].tolist())
        assert done and text.decode() in CHOICES
        # top_k = 0 takes the sampler's large path: the same guarantee
        big = llm.generate(inputs_embeds=e[:1], max_new_tokens=8, eos_token_id=EOS, constraint=c, seed=seed, do_sample=True, temperature=1.5, top_k=0, top_p=1.0)
        text, done = _text(big[0].tolist() + [EOS[0]])
        assert text.decode() in CHOICES, text


def test_mixed_batch_one_graph_any_automaton(automata):
    cfg, model, e, mask, lens = _tiny(57, False)
    llm, steps = model.llm, 100

    def run(con1, **open_kw):
        """Row 0 plain and live; after 3 steps row 1 joins with `con1`; -> (session, row 0's ids, row 1's ids)."""
        st = llm.batch_open(3, 256, 104, **open_kw)
        llm.batch_release(st, [0, 1, 2])
        f0 = llm.batch_admit(st, 0, e[0, :20])
        llm.batch_run(st, 3)
        f1 = llm.batch_admit(st, 1, e[1, :13], **({} if con1 is None else dict(constraint=con1)))
        llm.batch_run(st, steps)
        return st, [f0] + st.out_ids[0, :steps + 3].tolist(), [f1] + st.out_ids[1, :steps].tolist()

    st, a0, a1 = run(automata["choice"], constraints=True)
    graph = st.graph
    assert st.con is not None and "constraints" in st.key and graph is not None and st.con_state.tolist()[0] == -1
    text, done = _text(a1)
    assert done and text.decode() in CHOICES, a1
    st2, b0, b1 = run(automata["schema"], constraints=True)           # another automaton in the same slot: the same graph
    assert st2 is st and st.graph is graph and b0 == a0
    text, done = _text(b1)
    assert done and cn.dfa_accepts(automata["dfa"]["schema"], text), text
    _, c0, c1 = run(automata["choice"], constraints=True)             # and back: the request repeats its ids
    assert (c0, c1) == (a0, a1)
    _, d0, d1 = run(None, constraints=True)                           # an unconstrained newcomer ...
    stp, p0, p1 = run(None)                                           # ... gives the ids of a session without the flag, as row 0 does throughout
    assert stp is not st and stp.con is None and (d0, d1) == (p0, p1) and a0 == p0 and a1 != p1
    with pytest.raises(ValueError, match="constraints=True"):
        llm.batch_admit(stp, 1, e[1, :13], constraint=automata["choice"])
    with pytest.raises(ValueError, match="does not fit"):
        llm.batch_admit(llm.batch_open(3, 256, 104, constraints=True, max_states=4, max_classes=4), 1, e[1, :13], constraint=automata["schema"])


def test_constrained_row_beside_a_penalised_one_with_raw_logprobs(automata):
    from vila_amd import ops
    cfg, model, e, mask, lens = _tiny(59, False)
    llm, a, steps = model.llm, automata["schema"], 10
    st = llm.batch_open(3, 256, 16, penalties=True, logprobs=True, constraints=True)
    llm.batch_release(st, [0, 1, 2])
    f0 = llm.batch_admit(st, 0, e[0, :20], penalties=(1.0, 0.0, -1e4))
    f1 = llm.batch_admit(st, 1, e[1, :13], constraint=a)
    assert a.allowed(a.start)[f1]
    s, row0 = a.step(a.start, f1), [f0]
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(st.stream):
        for t in range(steps):
            llm._batch_step(st)
            st.stream.synchronize()
            tok = int(st.token[1])
            assert tok == masked_first_argmax(st.logits[1].cpu().numpy(), a.allowed(s)), t
            s = a.step(s, tok)
            # the record is RAW: the eager operator on the step's own raw logits gives the same bits, for the constrained and the penalised row
            tl, _, _ = ops.logprobs(st.logits[:2].clone(), st.token[:2].clone(), 0)
            assert torch.equal(_bits(st.lp_tok[:2, t]), _bits(tl)), t
            lse = torch.logsumexp(st.logits[1].double(), 0)
            assert abs(float(st.lp_tok[1, t]) - float(st.logits[1, tok].double() - lse)) < 1e-3
            row0.append(int(st.token[0]))
    assert all(row0[t] in row0[:t] for t in range(2, steps + 1)), row0      # the penalty acted on row 0


def test_shared_prefix_and_return_sequences(automata):
    cfg, model, e, mask, lens = _tiny(61, False)
    llm, a = model.llm, automata["schema"]
    ep = llm.embed_tokens(torch.randint(0, 900, (1, 300), generator=torch.Generator().manual_seed(3)).cuda())
    out = llm.generate(inputs_embeds=ep, max_new_tokens=N_NEW, eos_token_id=EOS, do_sample=True, temperature=1.2, top_k=30, top_p=0.95, seed=21,
                       batch_sample=True, num_return_sequences=3, constraint=a)
    st = llm._bdecode
    assert st.shared_prefix and st.S == 256 and st.con is not None and out.shape[0] == 3
    texts = set()
    for r in out.tolist():
        text, done = _text(r)
        assert done and cn.dfa_accepts(automata["dfa"]["schema"], text), text
        texts.add(text)
    assert len(texts) > 1, "three seeds gave one reply"
    # a sharing row admitted by hand, greedy, beside an unconstrained sharer
    st = llm.batch_open(2, 512, N_NEW, shared_prefix=True, constraints=True)
    llm.batch_release(st, [0, 1])
    assert llm.batch_set_prefix(st, ep[0]) == 256
    f0 = llm.batch_admit(st, 0, ep[0], share=True, constraint=automata["choice"])
    f1 = llm.batch_admit(st, 1, ep[0], share=True)
    llm.batch_run(st, 8)
    text, done = _text([f0] + st.out_ids[0, :8].tolist())
    assert done and text.decode() in CHOICES and st.con_state.tolist()[1] == -1


def test_continuous_batcher_admits_a_constrained_request_beside_a_running_plain_one(automata):
    import json
    import time as _t
    from tests.test_serving_cpu import _Tok
    from vila_amd import serving

    class Tok(_Tok):
        """Words in (the prompts), the synthetic vocabulary's bytes out (the replies)."""
        eos_token_id = EOS[0]

        def decode(self, ids, skip_special_tokens=True):
            return b"".join(TB[i] or b"" for i in ids).decode("utf-8", errors="replace")

    cfg, model, e, mask, lens = _tiny(63, False)
    tok = Tok()
    comp = cn.ConstraintCompiler(TB, EOS)
    fmt = {"type": "json_schema", "json_schema": {"name": "r", "schema": SCHEMA}}

    def serve(flag):
        kw = dict(constraints=True, compiler=comp) if flag else {}
        eng = serving.HipBatchEngine(model, tok, n_slots=4, max_ctx=256, max_new_tokens=N_NEW, eos_token_id=EOS, **kw)
        cb = serving.ContinuousBatcher(eng, max_batch=4, chunk=2, **(dict(constraints=True) if flag else {}))
        try:
            fa = cb.submit("describe the image in many words", 60)
            while not any(ev[0] == "run" for ev in cb.events):
                _t.sleep(0.001)
            if not flag:
                return cb, fa.result(timeout=120), None, None
            fb = cb.submit("what is this ?", 8, guided_choice=CHOICES)
            fc = cb.submit("read the fields", N_NEW, response_format=fmt)
            return cb, fa.result(timeout=120), fb.result(timeout=120), fc.result(timeout=120)
        finally:
            cb.close()

    cb, ta, tb, tc = serve(True)
    assert cb.constraints and model.llm._bdecode.con is not None and not any(ev[0] == "solo" for ev in cb.events)
    admits = [ev for ev in cb.events if ev[0] == "admit"]
    assert len(admits) == 3 and admits[1][2] > 0 and admits[1][3] >= 1, "the constrained request did not join a running batch"
    assert tb in CHOICES, tb
    assert cn.dfa_accepts(automata["dfa"]["schema2"], tc.encode()), tc
    assert list(json.loads(tc)) == ["name", "ok", "tags"]
    _, plain, _, _ = serve(False)
    assert model.llm._bdecode.con is None and plain == ta, "a constrained neighbour changed the plain request's reply"

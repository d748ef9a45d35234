"""Speculative decoding for penalised, constrained and logprob requests on the GPU (vila_llm_decode_step_verify_processed and its launches,
generate(spec_processed=True)).

Everything is exact.  The operators are compared bit for bit with the CPU chain references (tests/spec_processed_ref.py, which
tests/test_spec_processed_cpu.py pins to the sequential application of penalize_ref / constrain_ref); a session's ids, count table, automaton state and
logprob records are those of the same session drafting nothing; and every emitted id is recomputed on the CPU from the raw logits of its replay."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests import logprob_ref
from tests.constrain_ref import EOS_IDS, pairs_ref, synthetic_vocab
from tests.gpu_util import framed_operand, framed_out_rows, framed_ws
from tests.penalty_ref import counts_of, first_argmax, from_u16_bits, penalize_ref, u16_bits
from tests.spec_processed_ref import chain_counts, constrain_chain_ref, penalize_chain_ref
from tests.test_gpu_spec_decode import _exact_w4, _expected_trace
from vila_amd import _lib, configs, ops, synthetic
from vila_amd import constrain as cn
from vila_amd._lib import check

pytestmark = pytest.mark.gpu

PARAMS = [(1.3, 0.5, 0.25), (0.02, 0.0, 0.0), (1.0, -3.0, -1e4), (1.0, 0.0, 0.0)]
# (vocab, ld): 1003 / 1007 — unaligned rows, the scalar path; 4100 — the vector path, 129 + 3 indices per slice, so a 4-tail at the row's end and slices
# whose edges cut a thread's stride; 152064 — the model's
SHAPES = [(1003, 1007), (4100, 4100), (152064, 152064)]
CASES = [(n, V, ld) for V, ld in SHAPES[:2] for n in (2, 5, 16)] + [(16,) + SHAPES[2]]      # (the large vocabulary runs one row set)


def _dev(vals, dtype):
    return torch.tensor(vals, dtype=dtype, device="cuda")


def _bits(t):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if isinstance(t, torch.Tensor) else np.asarray(t)).contiguous().view(torch.int32)


def _tokens(V, n):
    """Index 0, V - 1, the two sides of a 4-chunk (3 | 4), an id twice (4) and three times (3), ids at counts 65534 / 65535 (twice each), -1 and V,
    both sides of the first slice edge; the first n of them."""
    per = (((V + 31) // 32) + 3) & ~3
    return [0, V - 1, 3, 4, 3, 3, -1, V, 100, 100, 101, 101, 4, per - 1, per, 0][:n]


def _logits(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, V, generator=g) * 3
    x[:, 9], x[:, 10], x[:, 11], x[:, 3], x[:, 100] = -0.0, float("inf"), float("-inf"), -2.5, -0.0
    x[0, 10] = 1.0                                                     # (one row whose maximum is finite)
    return x


def _check_pairs(pv, pi, y, what):
    wv, wi = pairs_ref(np.asarray(y), 32)
    assert np.array_equal(pv.cpu().numpy().view(np.int32), wv.view(np.int32)) and np.array_equal(pi.cpu().numpy(), wi), f"{what}: the (max, first index) pairs"


# ---- 1. the operators ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,V,ld", CASES)
def test_penalize_verify_is_bit_equal_to_the_cpu_chain(n, V, ld):
    x = _logits(n, V, 3 * n + V)
    g = torch.Generator().manual_seed(V)
    counts = torch.tensor([0, 1, 2, 65535])[torch.randint(0, 4, (V,), generator=g)]
    counts[100], counts[101], counts[0], counts[3], counts[4] = 65534, 65535, 0, 0, 7
    tokens = _tokens(V, n)
    lg = framed_operand(x.cuda(), ld_pad=ld - V, guard_rows=1, pad=1e9)           # 1e9 beyond the vocabulary: nothing there may be read
    cw = torch.full((V + 8,), 65535)
    cw[:V] = counts
    whole = u16_bits(cw).cuda()
    cnt, before = whole[:V], whole.clone()
    tok = _dev(tokens, torch.int64)
    for pen in PARAMS:
        out, frame = framed_out_rows(n, V, ld - V, 1, rows=n, dtype=torch.float32)
        y, pv, pi = ops.penalize_verify(lg, cnt, *(_dev([p], torch.float32) for p in pen), tok, out=out)
        torch.cuda.synchronize()
        want = penalize_chain_ref(x, counts, tokens, *pen)
        assert torch.equal(_bits(y), _bits(want)), (pen, int((_bits(y) != _bits(want)).sum()))
        frame()
        assert torch.equal(whole, before), "the launch must not write the count table"
        if pen == (1.0, 0.0, 0.0):
            assert torch.equal(_bits(y), _bits(x)), "neutral values copy the bits"
        _check_pairs(pv, pi, want, f"penalize_verify {pen}")
        for r in range(n):
            assert int(pi[r][pv[r] == pv[r].max()].min()) == first_argmax(want[r])
    # the repeated ids really count twice and three times, and the saturated ones stay
    assert int(chain_counts(counts, tokens, n - 1)[3]) == (3 if n > 5 else 2 if n > 4 else 1 if n > 2 else 0)
    if n == 16:
        assert chain_counts(counts, tokens, 15)[[100, 101, 4]].tolist() == [65535, 65535, 9]


@pytest.fixture(scope="module")
def autos():
    out = {}
    for V, _ in SHAPES + [(32000, 0), (1000, 0)]:
        comp = cn.ConstraintCompiler(synthetic_vocab() + [None] * (V - 1000), EOS_IDS)
        out[V] = dict(choice=comp.choice(["yes", "no!", "abc", "10 12"]), loop=comp.regex(r"(yes|no|ab|abc|bc|[ ,01]|12|100)+"))
    return out


def _con_dev(a, state):
    ld = (a.vocab + 3) // 4 * 4
    cls = torch.zeros(ld, dtype=torch.int16, device="cuda")
    cls[:a.vocab].copy_(torch.from_numpy(a.cls.view("int16")).cuda())
    return (_dev([state], torch.int32), cls, torch.from_numpy(a.next.reshape(-1).copy()).cuda(), _dev([a.n_classes], torch.int32))


@pytest.mark.parametrize("n,V,ld", CASES)
def test_constrain_verify_is_bit_equal_to_the_cpu_chain(autos, n, V, ld):
    tb = synthetic_vocab()
    b = lambda s: tb.index(s)
    x = _logits(n, V, 5 * n + V)
    # allowed bytes, a token the language forbids mid-chain (the state stays), ids out of range, a multi-byte token, duplicates, padding
    tokens = ([b(b"y"), b(b"e"), b(b"~1~"), b(b"s"), -1, V, b(b"1"), b(b"12"), b(b"12"), b(b","), b(b" "), b(b"abc"), V - 1, b(b"0")] + [b(b"y")] * 2)[:n]
    lg = framed_operand(x.cuda(), ld_pad=ld - V, guard_rows=1, pad=1e9)
    tok = _dev(tokens, torch.int64)
    for kind, a in autos[V].items():
        for start in (a.start, -1):
            state, cls, nxt, nc = _con_dev(a, start)
            out, frame = framed_out_rows(n, V, ld - V, 1, rows=n, dtype=torch.float32)
            y, states, pv, pi = ops.constrain_verify(lg, state, cls, nxt, nc, tok, out=out)
            torch.cuda.synchronize()
            want, want_states = constrain_chain_ref(x.numpy(), start, a.cls, a.next, a.n_classes, tokens)
            assert states.tolist() == want_states, (kind, start)
            assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32)), (kind, start)
            frame()
            assert state.tolist() == [start], "the launch must not write the state"
            _check_pairs(pv, pi, want, f"constrain_verify {kind} {start}")
            if start == -1:
                assert torch.equal(_bits(y), _bits(x)), "an unconstrained sequence copies the rows"
    if n >= 5:                                                         # the forbidden draft holds -inf in the row in front of it
        a = autos[V]["loop"]
        want, want_states = constrain_chain_ref(x.numpy(), a.start, a.cls, a.next, a.n_classes, tokens)
        assert want[1, tokens[2]] == -np.inf and want_states[2] == want_states[1]
    # in place: out may alias the logits
    a = autos[V]["loop"]
    state, cls, nxt, nc = _con_dev(a, a.start)
    buf = x.cuda().clone()
    y, _, _, _ = ops.constrain_verify(buf, state, cls, nxt, nc, tok, out=buf)
    want, _ = constrain_chain_ref(x.numpy(), a.start, a.cls, a.next, a.n_classes, tokens)
    assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("V", [1003, 4100])
def test_commit_bumps_what_the_step_consumed_and_moves_the_state(V):
    n = 16
    consumed = _tokens(V, n)
    states = list(range(40, 40 + n))
    start = torch.zeros(V, dtype=torch.int64)
    loaded = start.clone()
    loaded[100], loaded[101], loaded[3] = 65534, 65535, 65533
    for table in (start, loaded):
        for m in range(n):
            whole = u16_bits(torch.cat([table, torch.full((8,), 7)])).cuda()
            state = _dev([5], torch.int32)
            ops.verify_commit(V, _dev(consumed, torch.int64), _dev([m], torch.int32), counts=whole[:V], state=state, states=_dev(states, torch.int32))
            torch.cuda.synchronize()
            got = from_u16_bits(whole)
            assert torch.equal(got[:V], chain_counts(table, consumed, m)), (m, "the table behind the first m + 1 consumed ids")
            if table is start:
                assert torch.equal(got[:V], counts_of(consumed[:m + 1], V)[0])
            assert bool((got[V:] == 7).all()), "nothing beyond the vocabulary is written"
            assert state.tolist() == [states[m]]
    # m = 0 with padding rows that all repeat token[0]: one bump; counts alone and the state alone
    whole = u16_bits(start).cuda()
    ops.verify_commit(V, _dev([9] * n, torch.int64), _dev([0], torch.int32), counts=whole)
    assert torch.equal(from_u16_bits(whole), counts_of([9], V)[0])
    state = _dev([5], torch.int32)
    ops.verify_commit(V, _dev([9] * n, torch.int64), _dev([3], torch.int32), state=state, states=_dev(states, torch.int32))
    assert state.tolist() == [43]
    with pytest.raises(ValueError, match="neither"):
        ops.verify_commit(V, _dev([9] * n, torch.int64), _dev([0], torch.int32))


# ---- 2. one-sequence logprobs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1003, 32000])
def test_one_sequence_logprobs_write_the_accepted_rows_records(V):
    n, max_rec, m, old = 8, 12, 4, 6
    x = _logits(n, V, V + 1)
    x[:, 10] = 2.0
    token = [5, V - 1, 0, 77, 9, 1, 2, 3]
    rec = [old + i if i <= m else -1 for i in range(n)]
    rec[m] = max_rec                                                    # an index at max_rec: nothing is written
    lib = _lib.load()
    poison_t = torch.full((max_rec,), 123.0, device="cuda")
    poison_p = torch.full((max_rec, 20), 456.0, device="cuda")
    poison_i = torch.full((max_rec, 20), 789, device="cuda", dtype=torch.int32)
    tl, pl, pi = poison_t.clone(), poison_p.clone(), poison_i.clone()
    ws, ws_frame = framed_ws(lib.vila_logprobs_workspace_bytes(n))
    lg = x.cuda()
    out = _lib.VilaLogprobOut(tl.data_ptr(), pl.data_ptr(), pi.data_ptr(), max_rec)
    tok_d, rec_d = _dev(token, torch.int64), _dev(rec, torch.int32)
    check(lib.vila_logprobs_seq_f32(lg.data_ptr(), V, n, V, tok_d.data_ptr(), 20, rec_d.data_ptr(), C.byref(out), ws.data_ptr(), ops._stream()), "logprobs_seq")
    torch.cuda.synchronize()
    ws_frame()
    live = [i for i in range(n) if 0 <= rec[i] < max_rec]
    assert live == [0, 1, 2, 3]
    for i in live:
        t1, p1, i1 = ops.logprobs(lg[i:i + 1], _dev([token[i]], torch.int64), 20)
        k = rec[i]
        assert torch.equal(_bits(tl[k:k + 1]), _bits(t1)) and torch.equal(_bits(pl[k]), _bits(p1[0])) and torch.equal(pi[k], i1[0]), f"row {i}: the bits of the row alone"
    rows = torch.tensor(live)
    logprob_ref.check_rows(x[rows], torch.tensor(token)[rows], tl[[rec[i] for i in live]], pl[[rec[i] for i in live]], pi[[rec[i] for i in live]], 20)
    untouched = [k for k in range(max_rec) if k not in [rec[i] for i in live]]
    assert torch.equal(tl[untouched], poison_t[untouched]) and torch.equal(pl[untouched], poison_p[untouched]) and torch.equal(pi[untouched], poison_i[untouched])
    # the wrapper, and a refusal before any launch
    tl2, pl2, pi2 = poison_t.clone(), poison_p.clone(), poison_i.clone()
    ops.logprobs_seq(lg, tok_d, rec_d, tl2, pl2, pi2)
    assert torch.equal(_bits(tl2), _bits(tl)) and torch.equal(_bits(pl2), _bits(pl)) and torch.equal(pi2, pi)
    with pytest.raises(ValueError, match="record indices"):
        check(lib.vila_logprobs_seq_f32(lg.data_ptr(), V, n, V, tok_d.data_ptr(), 20, None, C.byref(out), ws.data_ptr(), ops._stream()), "seq")


# ---- 3. the session ------------------------------------------------------------------------------------------------------------------------------
N_NEW, S_PROMPT = 48, 300
# The synthetic model never repeats a token within 48 greedy tokens, so penalties that punish repeats change nothing.  These REWARD them (negative
# presence / frequency, OpenAI's range allows it): the reply starts to revisit its own tokens, counts pass 1, and lookup drafts repeat ids within a step.
# The session test asserts that the ids differ from the unpenalised ones.
PEN = (1.2, -6.0, -0.5)
PEN2 = (1.0, -2.0, 0.0)


def _8b():
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    return cfg


@pytest.fixture(scope="module")
def model_8b():
    from vila_amd.vlm import build_model
    return build_model(_8b(), seed=9)


@pytest.fixture(scope="module")
def prompt_8b(model_8b):
    g = torch.Generator().manual_seed(61)
    prompt = torch.randint(0, 31000, (S_PROMPT,), generator=g)
    llm = model_8b.llm
    e = llm.embed_tokens(prompt[None].cuda())
    plain = llm.generate(inputs_embeds=e, max_new_tokens=N_NEW, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=torch.empty(0, dtype=torch.int64))
    return prompt, e, plain[0].tolist()


class _Probe:
    """llm.spec_probe: after every replay, the emitted id of every row i <= m against the CPU chain applied to that replay's raw st.logits[i]."""

    def __init__(self, V, S, first, pen=None, auto=None, sampling=None):
        self.V, self.S, self.pen, self.auto, self.sampling = V, S, pen, auto, sampling
        self.ids, self.n_out, self.rows = [int(first)], 0, 0

    def __call__(self, st):
        m, n_out = int(st.n_accept), int(st.n_out)
        assert n_out == self.n_out + m + 1
        self.ids += st.out_ids[self.n_out:n_out].tolist()
        lg = st.logits[:m + 1].cpu()
        for i in range(m + 1):
            fed = self.ids[:self.n_out + i + 1]                         # everything consumed up to and including this row's token
            y = lg[i:i + 1]
            if self.pen is not None:
                y = penalize_ref(y, counts_of(fed, self.V), *self.pen)
            if self.auto is not None:
                s = self.auto.start
                for t in fed:
                    s = self.auto.step(s, t)
                y = torch.where(torch.from_numpy(self.auto.allowed(s))[None], y, torch.full_like(y, float("-inf")))
            if self.sampling is None:
                want = first_argmax(y[0])
            else:
                t_, k_, p_, seed = self.sampling
                want = int(ops.sample(y[0].cuda().contiguous(), t_, k_, p_, seed, counter=_dev([self.S + self.n_out + i], torch.int32)))
            assert self.ids[self.n_out + i + 1] == want, f"replay at n_out {self.n_out}, row {i}: emitted {self.ids[self.n_out + i + 1]}, the CPU chain gives {want}"
            self.rows += 1
        assert st.token[1:m + 1].tolist() == self.ids[self.n_out + 1:self.n_out + m + 1], "the accepted drafts are the ids the rows in front of them emitted"
        self.n_out = n_out


def _run(llm, e, k, probe_kw, **kw):
    """-> (ids, n_accept trace, logprobs or None, the probe)"""
    llm.spec_trace = []
    S = e.shape[1]
    box = {}

    def probe(st):
        if "p" not in box:
            # the first token is chosen eagerly: the session's token[0] before the first replay — recovered from the step's history
            box["p"] = _Probe(llm.lcfg.vocab_size, S, box["first"](st), **probe_kw)
        box["p"](st)
    # hist[n0 - 1] holds the first token (prompt_ids are not given in the probed runs' candidate mode; with a lookup the prompt comes first)
    box["first"] = lambda st: int(st.hist[int(kw["prompt_ids"].numel()) if kw.get("prompt_ids") is not None else 0])
    llm.spec_probe = probe
    try:
        out = llm.generate(inputs_embeds=e, max_new_tokens=N_NEW, eos_token_id=-1, prompt_lookup_num_tokens=k, spec_processed=True, **kw)
        lp = None
        if isinstance(out, tuple):
            out, lp = out
        return out[0].tolist(), list(llm.spec_trace), lp, box.get("p")
    finally:
        llm.spec_trace, llm.spec_probe = None, None


def _end_state(llm, ids, pen, auto):
    st = llm._vdecode
    n_out = int(st.n_out)
    fed = [ids[0]] + st.out_ids[:n_out - 1].tolist()
    if pen is not None:
        assert torch.equal(from_u16_bits(st.counts[0]), counts_of(fed, llm.lcfg.vocab_size)[0]), "the count table is not that of the consumed ids"
    if auto is not None:
        s = auto.start
        for t in fed:
            s = auto.step(s, t)
        assert int(st.con_state[0]) == s, "the automaton's state is not the CPU walk of the consumed ids"


def _lossless(llm, prompt, e, ks, gen, probe_kw):
    empty = torch.empty(0, dtype=torch.int64)
    ids0, tr0, lp0, p0 = _run(llm, e, 7, probe_kw, draft_ids=empty, **gen)
    assert len(ids0) == N_NEW and tr0 == [0] * (N_NEW - 1) and p0.rows == N_NEW - 1
    _end_state(llm, ids0, probe_kw.get("pen"), probe_kw.get("auto"))
    wrong = lambda t: (t + 1) % 31000
    at11 = list(ids0); at11[11] = wrong(at11[11])
    for k in ks:
        for name, cand in (("itself", ids0), ("corrupted at 11", at11), ("corrupted everywhere", [wrong(t) for t in ids0])):
            ids, tr, lp, p = _run(llm, e, k, probe_kw, draft_ids=torch.tensor(cand), **gen)
            print(f"k={k} candidate {name}: n_accept {tr}, {p.rows} rows checked")
            assert ids == ids0, f"k={k}, candidate {name}: the ids changed at index {next(i for i, (a, b) in enumerate(zip(ids, ids0)) if a != b)}"
            assert tr == _expected_trace(ids0, cand, k), f"k={k}, candidate {name}: n_accept {tr}"
            _end_state(llm, ids, probe_kw.get("pen"), probe_kw.get("auto"))
            if lp0 is not None:
                for a, b in zip(lp, lp0):
                    same = torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)
                    assert same, f"k={k}, candidate {name}: the records differ from the non-drafting session's"
        for hist in (prompt, torch.cat([prompt, torch.tensor(ids0)])):
            ids, tr, lp, p = _run(llm, e, k, probe_kw, prompt_ids=hist, **gen)
            print(f"k={k} lookup ({hist.numel()} ids of history): n_accept {tr}")
            assert ids == ids0, f"k={k}, lookup: the ids changed"
            _end_state(llm, ids, probe_kw.get("pen"), probe_kw.get("auto"))
    return ids0, lp0


def _gen_of(pen=None, auto=None, logprobs=None, sampling=None, any_top_k=False):
    gen = {}
    if pen is not None:
        gen.update(repetition_penalty=pen[0], presence_penalty=pen[1], frequency_penalty=pen[2])
    if auto is not None:
        gen.update(constraint=auto)
    if logprobs is not None:
        gen.update(logprobs=logprobs)
    if sampling is not None:
        gen.update(do_sample=True, spec_sample=True, temperature=sampling[0], top_k=sampling[1], top_p=sampling[2], seed=sampling[3])
        if any_top_k:
            gen.update(any_top_k=True)
    return gen


SESSIONS = {
    "penalties": dict(pen=PEN),
    "a choice list": dict(auto="choice"),
    "a regex": dict(auto="loop"),
    "penalties + regex": dict(pen=PEN, auto="loop"),
    "penalties + regex + logprobs": dict(pen=PEN, auto="loop", logprobs=5),
    "sampled + penalties": dict(pen=PEN, sampling=(0.7, 50, 0.9, 1234)),
    "any top_k + penalties": dict(pen=PEN, sampling=(0.7, 0, 0.9, 1234), any_top_k=True),
}


@pytest.mark.parametrize("name", list(SESSIONS))
def test_speculation_never_changes_a_processed_session(model_8b, prompt_8b, autos, name):
    """300-token prompt, 48 new tokens, k = 7 and 15: candidates equal to ids0, wrong at index 11 and wrong everywhere, and lookup drafts, all return the
    ids of the processed session drafting nothing, with the predicted n_accept of every replay, the end state of the consumed ids, the same record bits,
    and every emitted id equal to the CPU chain on its replay's raw logits."""
    llm = model_8b.llm
    prompt, e, plain = prompt_8b
    spec = dict(SESSIONS[name])
    auto = autos[32000][spec.pop("auto")] if "auto" in spec else None
    probe_kw = dict(pen=spec.get("pen"), auto=auto, sampling=spec.get("sampling"))
    ids0, lp0 = _lossless(llm, prompt, e, (7, 15), _gen_of(auto=auto, **spec), probe_kw)
    if spec.get("pen") is not None and spec.get("sampling") is None and auto is None:
        assert ids0 != plain, "the penalties must change the greedy ids within the 48 tokens, or the test shows nothing"
    if auto is not None:
        s = auto.start
        for t in ids0:
            assert auto.allowed(s)[t] or not auto.allowed(s).any(), "a token outside the language"
            s = auto.step(s, t)
    if lp0 is not None:
        assert lp0.token_logprobs.shape == (1, N_NEW) and lp0.top_ids.shape == (1, N_NEW, 5)


def test_a_second_request_reuses_the_graph_with_other_values(model_8b, prompt_8b, autos):
    llm = model_8b.llm
    prompt, e, _ = prompt_8b
    a1, a2 = autos[32000]["loop"], autos[32000]["choice"]
    ids1, _, _, _ = _run(llm, e, 7, dict(pen=PEN, auto=a1), prompt_ids=prompt, **_gen_of(pen=PEN, auto=a1))
    st, graph = llm._vdecode, llm._vdecode.graph
    assert graph is not None
    ids2, _, _, p2 = _run(llm, e, 7, dict(pen=PEN2, auto=a2), prompt_ids=prompt, **_gen_of(pen=PEN2, auto=a2))
    assert llm._vdecode is st and st.graph is graph, "the second request built a new session or captured a new graph"
    assert ids2 != ids1 and p2.rows >= N_NEW - 1, "the answers follow the new values (every row checked against the CPU chain with them)"
    _end_state(llm, ids2, PEN2, a2)
    ids3, _, _, _ = _run(llm, e, 7, dict(pen=PEN, auto=a1), prompt_ids=prompt, **_gen_of(pen=PEN, auto=a1))
    assert ids3 == ids1 and llm._vdecode.graph is graph
    # without the flag the old refusals stand
    with pytest.raises(ValueError, match="no penalised form"):
        llm.generate(inputs_embeds=e, max_new_tokens=4, prompt_lookup_num_tokens=7, repetition_penalty=1.1)


def test_step_entry_refuses_bad_arguments_before_any_launch(model_8b, prompt_8b):
    llm = model_8b.llm
    prompt, e, _ = prompt_8b
    llm.generate(inputs_embeds=e, max_new_tokens=4, eos_token_id=-1, prompt_lookup_num_tokens=7, spec_processed=True, repetition_penalty=1.1)
    st, lib = llm._vdecode, _lib.load()
    before = (st.pos.clone(), st.n_out.clone(), st.token.clone(), st.counts.clone())
    call = lambda c, ws_bytes, pen, sp=None, any_k=0: check(lib.vila_llm_decode_step_verify_processed(
        C.byref(llm._struct()), None, C.byref(st.cache.c), C.byref(c), st.ws.data_ptr(), ws_bytes, sp, any_k, pen, None, None, None), "step")
    bad = _lib.VilaDecodeVerify.from_buffer_copy(st.c)
    bad.n = 1
    with pytest.raises(ValueError, match="2..16 rows"):
        call(bad, st.ws.numel(), C.byref(st.pen))
    with pytest.raises(ValueError, match="workspace"):
        call(st.c, 4096, C.byref(st.pen))
    short = _lib.VilaPenalties(st.p_rep.data_ptr(), st.p_pres.data_ptr(), st.p_freq.data_ptr(), st.counts.data_ptr(), 100)
    with pytest.raises(ValueError, match="shorter than the vocabulary"):
        call(st.c, st.ws.numel(), C.byref(short))
    with pytest.raises(ValueError, match="any top_k"):
        call(st.c, st.ws.numel(), C.byref(st.pen), None, 1)
    torch.cuda.synchronize()
    for a, b in zip(before, (st.pos, st.n_out, st.token, st.counts)):
        assert torch.equal(a, b), "a refused step changed the state"


def test_step_entry_stays_inside_its_workspace(model_8b, prompt_8b, autos):
    """One eager step of the full chain — penalties, automaton, records — greedy and with the any-top_k draw, on a workspace of exactly the queried size
    between guards: nothing outside it is written, and the step moves the session by at least one token."""
    llm = model_8b.llm
    prompt, e, _ = prompt_8b
    auto = autos[32000]["loop"]
    llm.generate(inputs_embeds=e, max_new_tokens=4, eos_token_id=-1, prompt_lookup_num_tokens=7, spec_processed=True, logprobs=5, prompt_ids=prompt,
                 **_gen_of(pen=PEN, auto=auto))
    st, lib = llm._vdecode, _lib.load()
    assert st.pen is not None and st.con is not None and st.lp is not None
    nbytes = lib.vila_llm_decode_verify_processed_workspace_bytes(C.byref(llm._struct().shape), st.n, st.cache.max_ctx)
    assert nbytes == st.ws.numel()
    sp_t = (_dev([0.7], torch.float32), _dev([0], torch.int32), _dev([0.9], torch.float32), _dev([1234], torch.int64))
    sp = _lib.VilaBatchSampling(*(t.data_ptr() for t in sp_t))
    for sampled in (False, True):
        ws, frame = framed_ws(nbytes)
        n_out = int(st.n_out)
        check(lib.vila_llm_decode_step_verify_processed(C.byref(llm._struct()), None, C.byref(st.cache.c), C.byref(st.c), ws.data_ptr(), nbytes,
                                                        C.byref(sp) if sampled else None, 1 if sampled else 0, C.byref(st.pen), C.byref(st.con), C.byref(st.lp),
                                                        ops._stream()), "step")
        torch.cuda.synchronize()
        frame()
        assert int(st.n_out) == n_out + int(st.n_accept) + 1


# ---- 4. W4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_w4_session_is_lossless_with_penalties_and_an_automaton(autos):
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    for k in list(w):
        if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
            w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, (-7, -6, -5))
    llm = build_model(cfg, weights=w).llm
    llm.quantize_w4(batch_decode=True)
    g = torch.Generator().manual_seed(64)
    e = llm.embed_tokens(torch.randint(0, 900, (1, 300), generator=g).cuda())
    auto = autos[1000]["loop"]
    gen, probe_kw = _gen_of(pen=PEN, auto=auto), dict(pen=PEN, auto=auto)
    ids0, tr0, _, p0 = _run(llm, e, 7, probe_kw, draft_ids=torch.empty(0, dtype=torch.int64), **gen)
    assert llm._vdecode.w4 and tr0 == [0] * (N_NEW - 1)
    for cand in (ids0, [(t + 1) % 900 if i == 11 else t for i, t in enumerate(ids0)]):
        ids, tr, _, p = _run(llm, e, 7, probe_kw, draft_ids=torch.tensor(cand), **gen)
        assert ids == ids0 and tr == _expected_trace(ids0, cand, 7)
        _end_state(llm, ids, PEN, auto)


# ---- 5. the VLM, end to end ------------------------------------------------------------------------------------------------------------------------
def test_vlm_generate_with_a_choice_list_and_lookup_drafts(autos):
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    model = build_model(cfg, seed=0)
    px = synthetic.make_pixels(cfg, 1, 0).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, 12, 1, 0)
    media = {"image": [px[0].cuda()]}
    auto = autos[1000]["choice"]
    tb = synthetic_vocab()
    kw = dict(max_new_tokens=12, eos_token_id=list(EOS_IDS), constraint=auto, spec_processed=True, prompt_lookup_num_tokens=7)
    # the baseline is the same processed session drafting nothing (an empty candidate): the comparison is exact, no margin rule needed
    ref = model.generate(input_ids=ids[None], media=media, draft_ids=torch.empty(0, dtype=torch.int64), **kw)[0].tolist()
    out = model.generate(input_ids=ids[None], media=media, **kw)[0].tolist()
    assert out == ref
    assert out[-1] in EOS_IDS and b"".join(tb[t] for t in out[:-1]).decode() in ["yes", "no!", "abc", "10 12"], out

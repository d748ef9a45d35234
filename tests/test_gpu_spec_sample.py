"""Speculative decoding for sampled requests on the GPU (vila_llm_decode_step_verify_sample / _w4_sample, generate(spec_sample=True)): row i of
a step draws the token `ops.sample` returns for its logits with counter pos + i, and a draft is accepted exactly when it equals that draw — so,
whatever is drafted, the ids are bit for bit those of the same sampled session drafting nothing.  Every comparison here is an equality of ids."""
import ctypes as C
import zlib

import pytest
import torch

from tests.test_gpu_spec_decode import _8b, _Collect, _exact_w4, _expected_trace, _Slices
from vila_amd import _lib, configs, ops, serving, synthetic
from vila_amd._lib import check
from vila_amd.modules import _replay

pytestmark = pytest.mark.gpu

EMPTY = torch.empty(0, dtype=torch.int64)


@pytest.fixture(scope="module")
def model_8b():
    from vila_amd.vlm import build_model
    return build_model(_8b(), seed=9)


def _sampled(T=1.0, top_k=50, top_p=0.9, seed=1234):
    return dict(do_sample=True, temperature=T, top_k=top_k, top_p=top_p, seed=seed, spec_sample=True)


def _run(llm, e, n_new, k, sampling, **kw):
    """-> (ids, n_accept of every replay)"""
    llm.spec_trace = []
    try:
        out = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=k, **sampling, **kw)
        return out[0].tolist(), list(llm.spec_trace)
    finally:
        llm.spec_trace = None


# ---- 1. the draw is the sampler's ------------------------------------------------------------------------------------------------------------
def _draws_are_the_samplers(llm, e, w4):
    """One sampled step of n = 8 and of n = 16 rows whose drafts are the session's own continuation (every row accepted): out_ids[j] is the token
    ops.sample returns for logits row j with the request's parameters, seed and counter S + j, at 1.0 / 50 / 0.9.  At least one row must differ
    from its argmax for the test to tell a draw from a pick; were the synthetic logits too peaked for that at 1.0, the temperature is raised
    until the REFERENCE draws differ (a condition on the inputs; the equality is asserted at every temperature tried)."""
    S, seed = e.shape[1], 4242
    for T in (1.0, 2.0, 4.0, 8.0):
        sampling, differs = _sampled(T, 50, 0.9, seed), 0
        for n in (8, 16):
            ids0, _ = _run(llm, e, n + 1, n - 1, sampling, draft_ids=EMPTY)
            _, tr = _run(llm, e, 2, n - 1, sampling, draft_ids=torch.tensor(ids0))
            assert tr == [n - 1], f"T={T} n={n}: the session's own continuation was not accepted: {tr}"
            st = llm._vdecode
            assert st.sampled and st.n == n and st.w4 == w4 and st.s_temperature.numel() == 1
            out = st.out_ids[:n].tolist()
            assert out == ids0[1:]
            for j in range(n):
                ctr = torch.tensor([S + j], dtype=torch.int32, device="cuda")
                ref = int(ops.sample(st.logits[j], T, 50, 0.9, seed, counter=ctr))
                assert out[j] == ref, f"T={T} n={n} row {j}: step drew {out[j]}, ops.sample {ref}"
                differs += int(ref != int(st.logits[j].argmax()))
        print(f"T={T}: {differs} of 24 reference draws differ from the argmax of their row")
        if differs:
            return
    pytest.fail("the reference draws equal the argmax of every row up to temperature 8: these inputs cannot tell a draw from a pick")


def test_draw_is_the_samplers(model_8b):
    llm = model_8b.llm
    g = torch.Generator().manual_seed(71)
    _draws_are_the_samplers(llm, llm.embed_tokens(torch.randint(0, 31000, (1, 300), generator=g).cuda()), False)


@pytest.fixture(scope="module")
def llm_w4():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    for k in list(w):
        if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
            w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, (-7, -6, -5))
    llm = build_model(cfg, weights=w).llm
    llm.quantize_w4(batch_decode=True)
    return llm


def test_draw_is_the_samplers_w4(llm_w4):
    g = torch.Generator().manual_seed(72)
    _draws_are_the_samplers(llm_w4, llm_w4.embed_tokens(torch.randint(0, 900, (1, 300), generator=g).cuda()), True)


# ---- 2. speculation never changes sampled ids ------------------------------------------------------------------------------------------------
def _check_lossless(llm, prompt, n_new, ks, sampling):
    e = llm.embed_tokens(prompt[None].cuda())
    ids0, tr0 = _run(llm, e, n_new, 7, sampling, draft_ids=EMPTY)
    assert len(ids0) == n_new and tr0 == [0] * (n_new - 1), tr0
    assert llm._vdecode.sampled
    wrong = lambda t: (t + 1) % 31000
    at11 = list(ids0); at11[11] = wrong(at11[11])
    for k in ks:
        for name, cand in (("itself", ids0), ("corrupted at 11", at11), ("corrupted everywhere", [wrong(t) for t in ids0])):
            ids, tr = _run(llm, e, n_new, k, sampling, draft_ids=torch.tensor(cand))
            want = _expected_trace(ids0, cand, k)
            print(f"k={k} candidate {name}: n_accept {tr}")
            assert ids == ids0, f"k={k}, candidate {name}: the ids changed at index {next(i for i, (a, b) in enumerate(zip(ids, ids0)) if a != b)}"
            assert tr == want, f"k={k}, candidate {name}: n_accept {tr}, expected {want}"
        ids, tr = _run(llm, e, n_new, k, sampling, prompt_ids=prompt)
        assert ids == ids0, f"k={k}, lookup in the prompt: the ids changed"
        ids, tr = _run(llm, e, n_new, k, sampling, prompt_ids=torch.cat([prompt, torch.tensor(ids0)]))
        print(f"k={k} lookup with the answer in the history: n_accept {tr}")
        assert ids == ids0, f"k={k}, lookup with the answer in the history: the ids changed"
    return e, ids0


def test_speculation_never_changes_sampled_ids(model_8b):
    """300-token prompt, 48 new tokens at 1.0 / 50 / 0.9.  ids0: the sampled verify session that drafts nothing.  Candidates equal to ids0, wrong at
    index 11 and wrong everywhere, and lookup drafts, with k = 7 and k = 15, all return ids0 bit for bit, with the n_accept of every replay as
    predicted.  The session samples: ids0 is not the greedy verify session's output, and another seed gives other ids."""
    llm = model_8b.llm
    g = torch.Generator().manual_seed(61)
    prompt = torch.randint(0, 31000, (300,), generator=g)
    e, ids0 = _check_lossless(llm, prompt, 48, (7, 15), _sampled(seed=1234))
    assert _expected_trace(ids0, ids0, 7) == [7] * 6
    greedy = llm.generate(inputs_embeds=e, max_new_tokens=48, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=EMPTY)[0].tolist()
    assert not llm._vdecode.sampled
    assert ids0 != greedy, "the sampled session returned the greedy ids"
    other, _ = _run(llm, e, 48, 7, _sampled(seed=1235), draft_ids=EMPTY)
    assert other != ids0, "a second seed gave the same ids"


@pytest.mark.parametrize("force", [0, 2])
def test_speculation_never_changes_sampled_ids_walking_cache(model_8b, force):
    """The same over a 2300-token prompt (a 2560-position cache: slices walk; force 2: 5 chunks per slice).  The graph bakes the slice count, so the
    session is dropped around the hook."""
    llm = model_8b.llm
    g = torch.Generator().manual_seed(62)
    prompt = torch.randint(0, 31000, (2300,), generator=g)
    llm._drop_session("_vdecode")
    try:
        with _Slices(force):
            _check_lossless(llm, prompt, 48, (7, 15), _sampled(seed=99))
            assert llm._vdecode.cache.max_ctx == 2560
    finally:
        llm._drop_session("_vdecode")


# ---- 3. top_k = 1 is greedy ------------------------------------------------------------------------------------------------------------------
def test_top_k_1_and_a_non_positive_temperature_are_greedy(model_8b):
    llm = model_8b.llm
    g = torch.Generator().manual_seed(73)
    e = llm.embed_tokens(torch.randint(0, 31000, (1, 300), generator=g).cuda())
    S, n_new = 300, 17
    ids_g = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7)[0].tolist()
    ids_1 = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7, **_sampled(1.0, 1, 0.9, 5))[0].tolist()
    assert ids_1 == ids_g
    # step level: the sampled session's graph with a temperature entry <= 0 — every row is a greedy row whatever top_k / top_p / seed say.  The
    # cache still holds the prompt; the candidate is the greedy output, so two replays accept 7 drafts each and emit its 16 tokens.
    st = llm._vdecode
    assert st.sampled and st.graph is not None
    cand = torch.tensor(ids_g[1:], dtype=torch.int64, device="cuda")
    for T in (0.0, -1.0):
        llm._verify_set_sampling(st, (T, 50, 0.9, 5))
        st.cand[:cand.numel()].copy_(cand)
        st.n_cand.fill_(cand.numel())
        st.pos.fill_(S); st.n_out.zero_(); st.n_hist.fill_(1); st.token[:1].fill_(ids_g[0])
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(st.stream):
            _replay(st, 2)
        st.stream.synchronize()
        assert int(st.n_out) == 16 and int(st.n_accept) == 7 and int(st.pos) == S + 16
        assert st.out_ids[:16].tolist() == ids_g[1:], f"temperature {T}: the rows did not pick greedily"


# ---- 4. sessions -----------------------------------------------------------------------------------------------------------------------------
def test_sessions(model_8b):
    from vila_amd.vlm import build_model
    llm = model_8b.llm
    g = torch.Generator().manual_seed(74)
    prompt = torch.randint(0, 31000, (1, 300), generator=g)
    e = llm.embed_tokens(prompt.cuda())
    kw = dict(inputs_embeds=e, max_new_tokens=24, eos_token_id=-1, prompt_lookup_num_tokens=7, prompt_ids=prompt[0])
    req1, req2 = _sampled(0.8, 50, 0.9, 11), _sampled(1.3, 50, 0.7, 12)
    g1 = llm.generate(**kw)[0].tolist()
    s1 = llm.generate(**kw, **req1)[0].tolist()
    graph = llm._vdecode.graph
    assert llm._vdecode.sampled and graph is not None
    s2 = llm.generate(**kw, **req2)[0].tolist()
    assert llm._vdecode.graph is graph, "the second sampled request captured a new graph"
    assert s2 != s1
    g3 = llm.generate(**kw)[0].tolist()
    assert not llm._vdecode.sampled and g3 == g1 and s1 != g1
    # the second request alone on a fresh model: nothing of the first request was left in the graph or the session
    fresh = build_model(_8b(), seed=9).llm
    assert fresh.generate(**dict(kw, inputs_embeds=fresh.embed_tokens(prompt.cuda())), **req2)[0].tolist() == s2


# ---- 5. top level ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_vlm():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    return cfg, build_model(cfg, seed=0)


def test_vlm_generate_with_lookup_drafts_sampled(tiny_vlm):
    cfg, model = tiny_vlm
    llm = model.llm
    px = synthetic.make_pixels(cfg, 1, 0).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, 12, 1, 0)
    media = {"image": [px[0].cuda()]}
    e, _, _ = model._embed(ids[None], {"image": [px[0].cuda()]})
    n_new, req = 24, _sampled(1.0, 50, 0.9, 77)
    ref = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=EMPTY, **req)[0].tolist()
    graph = llm._vdecode.graph
    greedy = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1)[0].tolist()
    assert ref != greedy
    out = model.generate(input_ids=ids[None], media=media, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7, **req)
    assert out.shape == (1, n_new) and out[0].tolist() == ref
    assert llm._vdecode.graph is graph, "the second request captured a new graph"
    # the solo sampled session draws the same first token (same logits, same counter S - 1)
    assert llm.generate(inputs_embeds=e, max_new_tokens=1, eos_token_id=-1, do_sample=True, temperature=1.0, top_k=50, top_p=0.9, seed=77)[0].tolist() == ref[:1]
    # EOS inside an accepted run cuts the output there (HF: the EOS is the last token)
    j = next(i for i in range(3, n_new) if ref.index(ref[i]) == i)
    cut = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=ref[j], prompt_lookup_num_tokens=7, draft_ids=torch.tensor(ref), **req)
    assert cut[0].tolist() == ref[:j + 1]
    # max_new_tokens that is no multiple of k + 1, with every draft accepted; the streamer sees each token once, in order
    s = _Collect()
    out13 = llm.generate(inputs_embeds=e, max_new_tokens=13, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=torch.tensor(ref), streamer=s, **req)
    assert out13[0].tolist() == ref[:13] and s.toks == ref[:13] and s.ended == 1
    s = _Collect()
    model.generate(input_ids=ids[None], media=media, max_new_tokens=n_new, eos_token_id=ref[j], prompt_lookup_num_tokens=7, streamer=s, **req)
    assert s.toks == ref[:j + 1] and s.ended == 1
    assert llm.generate(inputs_embeds=e, max_new_tokens=1, eos_token_id=-1, prompt_lookup_num_tokens=7, **req)[0].tolist() == ref[:1]
    # after a chunked prefill (its logits are another prefill's: a reference of its own) drafts change nothing either
    assert e.shape[1] > 8
    chunked = dict(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7, prefill_chunk=8, **req)
    ref_c = llm.generate(draft_ids=EMPTY, **chunked)[0].tolist()
    assert llm.generate(draft_ids=torch.tensor(ref_c), **chunked)[0].tolist() == ref_c


class _WordTok:
    """Whitespace tokenizer over a fixed vocabulary; ids it does not know decode to a placeholder."""
    eos_token_id = 2

    def __init__(self):
        words = ["<unk>", "<|im_start|>", "<|im_end|>", "system", "user", "assistant", "what", "is", "this", "?", "and", "the", "colour"]
        self.vocab = {w: i for i, w in enumerate(words)}

    def __call__(self, text, add_special_tokens=False):
        from types import SimpleNamespace
        return SimpleNamespace(input_ids=[self.vocab.get(w, 0) for w in text.split()])

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"w{i}" for i in ids)


def test_chat_session_follow_up_turn_speculates_sampled(tiny_vlm):
    """Two sessions share a greedy first turn; the follow-up turn is the same sampled request, once drafting nothing (an empty candidate) and once
    with lookup drafts: the ids are equal."""
    import numpy as np
    cfg, model = tiny_vlm
    tok = _WordTok()
    img = np.random.default_rng(3).integers(0, 256, size=(56, 56, 3), dtype=np.uint8)
    req = _sampled(1.0, 50, 0.9, 31)
    a = serving.ChatSession(model, tok, max_ctx=256, eos_token_id=-1)
    b = serving.ChatSession(model, tok, max_ctx=256, eos_token_id=-1)
    for s in (a, b):
        s.ask([img, "what is this ?"], max_new_tokens=6)
    assert a.ids == b.ids and a.cached == b.cached > 0
    a.ask("and the colour ?", max_new_tokens=12, prompt_lookup_num_tokens=7, draft_ids=EMPTY, **req)
    b.ask("and the colour ?", max_new_tokens=12, prompt_lookup_num_tokens=7, **req)
    assert model.llm._vdecode.sampled
    assert b.ids == a.ids and b.cached == a.cached
    c = serving.ChatSession(model, tok, max_ctx=256, eos_token_id=-1)
    c.ask([img, "what is this ?"], max_new_tokens=6)
    c.ask("and the colour ?", max_new_tokens=12)
    assert c.ids[:-12] == a.ids[:-12] and c.ids != a.ids, "the sampled follow-up turn returned the greedy ids"


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(tiny_vlm):
    from vila_amd.vlm import build_model
    llm = tiny_vlm[1].llm
    g = torch.Generator().manual_seed(75)
    e = llm.embed_tokens(torch.randint(0, 900, (2, 20), generator=g).cuda())
    kw = dict(max_new_tokens=4, prompt_lookup_num_tokens=3)
    for k in (0, 65):
        with pytest.raises(ValueError, match="top_k"):
            llm.generate(inputs_embeds=e[:1], **kw, **_sampled(top_k=k))
    with pytest.raises(ValueError, match="batch size 1"):
        llm.generate(inputs_embeds=e, **kw, **_sampled())
    big = llm.new_cache(llm.BATCH_MAX_CTX + 256)
    with pytest.raises(ValueError, match="caches up to"):
        llm.generate(inputs_embeds=e[:1], cache=big, **kw, **_sampled())
    del big
    qcfg = configs.tiny("mlp_downsample")
    qcfg.llm.intermediate_size = 1152                           # a multiple of the 128-wide quantisation group
    q = build_model(qcfg, seed=0).llm
    q.quantize_w4()
    with pytest.raises(ValueError, match="batch_decode=True"):
        q.generate(inputs_embeds=e[:1], **kw, **_sampled())
    # the mode still serves the request it refused nothing of
    assert llm.generate(inputs_embeds=e[:1], eos_token_id=-1, **kw, **_sampled()).shape == (1, 4)
    # the C entry names its restrictions before anything is enqueued: the greedy step's workspace is too small for it, and it needs its parameters
    st, lib, w = llm._vdecode, _lib.load(), llm._struct()
    greedy_bytes = lib.vila_llm_decode_verify_workspace_bytes(C.byref(w.shape), st.n, st.cache.max_ctx)
    assert st.sampled and greedy_bytes < st.ws.numel()
    before = (st.pos.clone(), st.n_out.clone(), st.token.clone())
    with pytest.raises(ValueError, match="workspace too small"):
        check(lib.vila_llm_decode_step_verify_sample(C.byref(w), C.byref(st.cache.c), C.byref(st.c), st.ws.data_ptr(), greedy_bytes, C.byref(st.sp), None), "step")
    with pytest.raises(ValueError, match="sampling parameters are NULL"):
        check(lib.vila_llm_decode_step_verify_sample(C.byref(w), C.byref(st.cache.c), C.byref(st.c), st.ws.data_ptr(), st.ws.numel(), None, None), "step")
    torch.cuda.synchronize()
    for x, y in zip(before, (st.pos, st.n_out, st.token)):
        assert torch.equal(x, y), "a refused step changed the state"

"""Greedy speculative decoding on the GPU (vila_llm_decode_step_verify, bdec_attn_shared_kernel, generate(prompt_lookup_num_tokens=)): the
shared-KV attention against an fp32 softmax, the draft kernel against its host reference, and the property the feature stands on — whatever is
drafted, the ids are those of the session that drafts nothing."""
import ctypes as C
import zlib

import pytest
import torch

from tests.gpu_util import rel_l2
from tests.test_spec_decode_cpu import DRAFT_CASES
from vila_amd import _lib, configs, ops, synthetic
from vila_amd._lib import check
from vila_amd.host import prompt_lookup_draft

pytestmark = pytest.mark.gpu


class _Slices:
    """vila_decode_batch_force_slices for a `with` block; always back to automatic."""

    def __init__(self, nsl):
        self.nsl = nsl

    def __enter__(self):
        _lib.load().vila_decode_batch_force_slices(int(self.nsl))

    def __exit__(self, *a):
        _lib.load().vila_decode_batch_force_slices(0)


# ---- a. the kernel against fp32 --------------------------------------------------------------------------------------------------------
MAX_CTX, KV = 4096, 2
# (n, pos): one key; rows straddle a wave's 16-key piece; rows straddle a 256-key chunk; a partial last column tile at G = 7 (35 columns); the last
# row on the last position with 16 chunks walked; rows past the capacity (clamped to the last key)
CASES = [(1, 0), (16, 7), (16, 250), (5, 2047), (16, 4080), (16, 4090)]


@pytest.fixture(scope="module")
def kv_slot():
    g = torch.Generator().manual_seed(5)
    k = torch.randn((KV, MAX_CTX, 128), generator=g).to(torch.bfloat16).cuda()
    v = torch.randn((KV, MAX_CTX, 128), generator=g).to(torch.bfloat16).cuda()
    return k, v, k.float(), v.float()


@pytest.mark.parametrize("G", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("force", [0, 3])
def test_shared_attention_against_fp32_softmax(kv_slot, G, force):
    """max|o - ref| <= 2^-7 max|V| with the per-row key limit min(pos + i, max_ctx - 1): the bound and rationale of
    test_walking_attention_against_fp32_softmax (a convex combination of V rows rounded once to bf16, relative 2^-9, times 4 for __expf and the
    summation order; here P is bf16 on the matrix core, another 2^-9 inside the same factor).  force 0: 8 slices of up to 2 chunks; 3: up to 6."""
    k, v, kf, vf = kv_slot
    scale = 128 ** -0.5
    g = torch.Generator().manual_seed(200 + G)
    bound = 2.0 ** -7 * float(vf.abs().max())
    with _Slices(force):
        for n, p in CASES:
            q = torch.randn((n, KV * G, 128), generator=g).to(torch.bfloat16).cuda()
            pos = torch.tensor([p], dtype=torch.int32, device="cuda")
            o = ops.attn_decode_verify(q, k, v, pos, scale)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(o.float()).all()), f"G={G} force={force} n={n} pos={p}: non-finite output"
            for i in range(n):
                L = min(p + i, MAX_CTX - 1) + 1
                s = torch.einsum("hd,hld->hl", q[i].float(), kf[:, :L].repeat_interleave(G, 0)) * scale
                ref = torch.einsum("hl,hld->hd", torch.softmax(s, -1), vf[:, :L].repeat_interleave(G, 0))
                err = float((o[i].float() - ref).abs().max())
                if i in (0, n - 1):
                    print(f"G={G} force={force} n={n} pos={p} row {i}: max|o - ref| = {err:.3e} (bound {bound:.3e})")
                assert err <= bound, f"G={G} force={force} n={n} pos={p} row {i} ({L} keys): {err:.3e} > {bound:.3e}"


def test_shared_attention_row_does_not_depend_on_the_step(kv_slot):
    """The invariance the feature stands on, at operator level: the row at position p gives the same bits alone (n = 1), as row 3 of 5 and as row 15
    of 16 (another column tile, another block of the tile groups at G = 7)."""
    k, v, _, _ = kv_slot
    g = torch.Generator().manual_seed(77)
    q = torch.randn((16, KV * 7, 128), generator=g).to(torch.bfloat16).cuda()
    for p in (300, 2600):
        i32 = lambda x: torch.tensor([x], dtype=torch.int32, device="cuda")
        full = ops.attn_decode_verify(q, k, v, i32(p - 15))
        alone = ops.attn_decode_verify(q[15:16], k, v, i32(p))
        mid = ops.attn_decode_verify(q[12:], k, v, i32(p - 3))
        assert torch.equal(full[15], alone[0]) and torch.equal(full[15], mid[3])


# ---- b. the draft kernel ---------------------------------------------------------------------------------------------------------------
def test_draft_kernel_equals_the_host_reference():
    cases = [(ids, k, ng) for ids, k, ng, _ in DRAFT_CASES]
    g = torch.Generator().manual_seed(11)
    for _ in range(50):
        L = int(torch.randint(1, 601, (1,), generator=g))
        cases.append((torch.randint(0, 5, (L,), generator=g).tolist(), int(torch.randint(1, 16, (1,), generator=g)), int(torch.randint(1, 5, (1,), generator=g))))
    for ids, k, ng in cases:
        hist = torch.tensor(ids + [4] * 7, dtype=torch.int64).cuda()      # ids past n_hist must not be seen
        assert ops.prompt_lookup_draft(hist, len(ids), k, ng) == prompt_lookup_draft(ids, k, ng), (ids, k, ng)


# ---- c. speculation never changes the ids ----------------------------------------------------------------------------------------------
def _8b():
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    return cfg


@pytest.fixture(scope="module")
def model_8b():
    from vila_amd.vlm import build_model
    return build_model(_8b(), seed=9)


def _run(llm, e, n_new, k, **kw):
    """-> (ids, n_accept of every replay)"""
    llm.spec_trace = []
    try:
        out = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=k, **kw)
        return out[0].tolist(), list(llm.spec_trace)
    finally:
        llm.spec_trace = None


def _expected_trace(ids0, cand, k):
    """n_accept of every replay when the model's own tokens are ids0 and the candidate output is cand (both include the prefill's token)."""
    out, c, n_out, trace = ids0[1:], cand[1:], 0, []
    while n_out < len(out):
        nd = min(k, max(0, len(c) - n_out))
        m = 0
        while m < nd and out[n_out + m] == c[n_out + m]:
            m += 1
        trace.append(m)
        n_out += m + 1
    return trace


def _check_lossless(llm, prompt, n_new, ks):
    e = llm.embed_tokens(prompt[None].cuda())
    empty = torch.empty(0, dtype=torch.int64)
    ids0, tr0 = _run(llm, e, n_new, 7, draft_ids=empty)
    assert len(ids0) == n_new and tr0 == [0] * (n_new - 1), tr0
    wrong = lambda t: (t + 1) % 31000
    at11 = list(ids0); at11[11] = wrong(at11[11])
    for k in ks:
        for name, cand in (("itself", ids0), ("corrupted at 11", at11), ("corrupted everywhere", [wrong(t) for t in ids0])):
            ids, tr = _run(llm, e, n_new, k, draft_ids=torch.tensor(cand))
            want = _expected_trace(ids0, cand, k)
            print(f"k={k} candidate {name}: n_accept {tr}")
            assert ids == ids0, f"k={k}, candidate {name}: the ids changed at index {next(i for i, (a, b) in enumerate(zip(ids, ids0)) if a != b)}"
            assert tr == want, f"k={k}, candidate {name}: n_accept {tr}, expected {want}"
        ids, tr = _run(llm, e, n_new, k, prompt_ids=prompt)
        assert ids == ids0, f"k={k}, lookup in the prompt: the ids changed"
        # a history that already holds the answer: the lookup finds it and drafts that are right get accepted
        ids, tr = _run(llm, e, n_new, k, prompt_ids=torch.cat([prompt, torch.tensor(ids0)]))
        print(f"k={k} lookup with the answer in the history: n_accept {tr}")
        assert ids == ids0, f"k={k}, lookup with the answer in the history: the ids changed"
    return ids0


def test_speculation_never_changes_the_ids(model_8b):
    """300-token prompt, 48 new tokens.  ids0: the verify session that drafts nothing (an empty candidate).  Candidates equal to ids0, wrong at index
    11 and wrong everywhere, and lookup drafts, with k = 7 and k = 15, all return ids0 bit for bit, with the n_accept of every replay as predicted."""
    llm = model_8b.llm
    g = torch.Generator().manual_seed(61)
    prompt = torch.randint(0, 31000, (300,), generator=g)
    ids0 = _check_lossless(llm, prompt, 48, (7, 15))
    assert _expected_trace(ids0, ids0, 7) == [7] * 6
    at11 = list(ids0); at11[11] = -1
    assert _expected_trace(ids0, at11, 7)[:3] == [7, 2, 7]             # tokens per replay: 8, 3, then 8 ...


@pytest.mark.parametrize("force", [0, 2])
def test_speculation_never_changes_the_ids_walking_cache(model_8b, force):
    """The same over a 2300-token prompt (a 2560-position cache: slices walk; force 2: 5 chunks per slice).  The graph bakes the slice count, so the
    session is dropped around the hook."""
    llm = model_8b.llm
    g = torch.Generator().manual_seed(62)
    prompt = torch.randint(0, 31000, (2300,), generator=g)
    llm._drop_session("_vdecode")
    try:
        with _Slices(force):
            _check_lossless(llm, prompt, 48, (7, 15))
            assert llm._vdecode.cache.max_ctx == 2560
    finally:
        llm._drop_session("_vdecode")


# ---- d. the step's rows against solo runs ----------------------------------------------------------------------------------------------
def _rows_vs_solo(llm, e, tol=1.5e-2):
    """One verify step of 8 rows fed the solo greedy continuation: every row's logits against the solo teacher-forced logits of its position
    (rel_l2 < 1.5e-2) and its pick under the margin rule — the tolerances of test_long_batch_rows_against_their_solo_runs."""
    ids, lgs = llm.generate(inputs_embeds=e, max_new_tokens=9, return_logits=True, use_graph=False, eos_token_id=-1)
    ids = ids[0]
    llm.spec_trace = []
    try:
        llm.generate(inputs_embeds=e, max_new_tokens=2, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=ids)
        assert len(llm.spec_trace) == 1
    finally:
        llm.spec_trace = None
    st = llm._vdecode
    assert st.token[1:].tolist() == ids[1:8].tolist() and int(st.n_draft) == 7
    top2 = lgs.float().topk(2, -1).values
    margin, bound = (top2[:, 0] - top2[:, 1]).cpu(), 4 * tol * float(lgs.float().abs().max())
    for i in range(8):
        rel = rel_l2(st.logits[i], lgs[i + 1])
        print(f"row {i}: logits rel_l2 = {rel:.3e}")
        assert rel < tol, f"row {i}: rel={rel:.3e}"
    for i in range(8):
        if int(st.logits[i].argmax()) != int(ids[i + 1]):
            assert float(margin[i + 1]) <= bound, f"row {i}: pick {int(st.logits[i].argmax())} vs solo {int(ids[i + 1])} at a decisive step"
            break


def test_verify_rows_against_solo_runs(model_8b):
    llm = model_8b.llm
    g = torch.Generator().manual_seed(63)
    _rows_vs_solo(llm, llm.embed_tokens(torch.randint(0, 31000, (1, 300), generator=g).cuda()))


def _exact_w4(shape, seed, log2_scale):
    """Weights that int4 groups of 128 represent exactly (as tests/test_gpu_w4_batch_decode.py builds them)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-8, 8, shape, generator=g).float()
    e = torch.tensor(log2_scale, dtype=torch.float32)[torch.randint(0, len(log2_scale), (shape[0], shape[1] // 128), generator=g)]
    return (q.view(shape[0], -1, 128) * torch.exp2(e)[..., None]).view(shape)


def test_verify_rows_against_solo_runs_w4():
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
    _rows_vs_solo(llm, llm.embed_tokens(torch.randint(0, 900, (1, 300), generator=g).cuda()))
    assert llm._vdecode.w4


# ---- e. end to end ---------------------------------------------------------------------------------------------------------------------
class _Collect:
    def __init__(self):
        self.toks, self.ended = [], 0

    def put(self, t):
        assert t.shape == (1,)
        self.toks.append(int(t))

    def end(self):
        self.ended += 1


def test_vlm_generate_with_lookup_drafts():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    model = build_model(cfg, seed=0)
    llm = model.llm
    px = synthetic.make_pixels(cfg, 1, 0).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, 12, 1, 0)
    media = {"image": [px[0].cuda()]}
    e, _, _ = model._embed(ids[None], {"image": [px[0].cuda()]})
    n_new = 24
    ref = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=torch.empty(0, dtype=torch.int64))[0].tolist()
    graph = llm._vdecode.graph
    out = model.generate(input_ids=ids[None], media=media, max_new_tokens=n_new, eos_token_id=-1, prompt_lookup_num_tokens=7)
    assert out.shape == (1, n_new) and out[0].tolist() == ref
    assert llm._vdecode.graph is graph, "the second request captured a new graph"
    # EOS inside an accepted run cuts the output there (HF: the EOS is the last token)
    j = next(i for i in range(3, n_new) if ref.index(ref[i]) == i)
    cut = llm.generate(inputs_embeds=e, max_new_tokens=n_new, eos_token_id=ref[j], prompt_lookup_num_tokens=7, draft_ids=torch.tensor(ref))
    assert cut[0].tolist() == ref[:j + 1]
    # max_new_tokens that is no multiple of k + 1, with every draft accepted; the streamer sees each token once, in order
    s = _Collect()
    out13 = llm.generate(inputs_embeds=e, max_new_tokens=13, eos_token_id=-1, prompt_lookup_num_tokens=7, draft_ids=torch.tensor(ref), streamer=s)
    assert out13[0].tolist() == ref[:13] and s.toks == ref[:13] and s.ended == 1
    s = _Collect()
    model.generate(input_ids=ids[None], media=media, max_new_tokens=n_new, eos_token_id=ref[j], prompt_lookup_num_tokens=7, streamer=s)
    assert s.toks == ref[:j + 1] and s.ended == 1
    assert llm.generate(inputs_embeds=e, max_new_tokens=1, eos_token_id=-1, prompt_lookup_num_tokens=7)[0].tolist() == ref[:1]


# ---- f. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(model_8b):
    from vila_amd.vlm import build_model
    llm = model_8b.llm
    g = torch.Generator().manual_seed(65)
    e = llm.embed_tokens(torch.randint(0, 31000, (1, 300), generator=g).cuda())
    with pytest.raises(ValueError, match="KV cache too small"):
        llm.generate(inputs_embeds=e, max_new_tokens=8, prompt_lookup_num_tokens=7, cache=llm.new_cache(256))
    # the C entry names its restrictions before anything is enqueued
    llm.generate(inputs_embeds=e, max_new_tokens=2, eos_token_id=-1, prompt_lookup_num_tokens=7)
    st, lib = llm._vdecode, _lib.load()
    before = (st.pos.clone(), st.n_out.clone(), st.token.clone())
    bad = _lib.VilaDecodeVerify.from_buffer_copy(st.c)
    bad.n = 1
    with pytest.raises(ValueError, match="2..16 rows"):
        check(lib.vila_llm_decode_step_verify(C.byref(llm._struct()), C.byref(st.cache.c), C.byref(bad), st.ws.data_ptr(), st.ws.numel(), None), "step")
    with pytest.raises(ValueError, match="workspace too small"):
        check(lib.vila_llm_decode_step_verify(C.byref(llm._struct()), C.byref(st.cache.c), C.byref(st.c), st.ws.data_ptr(), 4096, None), "step")
    torch.cuda.synchronize()
    for a, b in zip(before, (st.pos, st.n_out, st.token)):
        assert torch.equal(a, b), "a refused step changed the state"
    # a model whose q/k/v are no longer one buffer
    tiny = build_model(configs.tiny("mlp_downsample"), seed=0).llm
    a = getattr(tiny.model.layers, "0").self_attn
    a.k_proj.weight.data = a.k_proj.weight.data.clone()
    et = tiny.embed_tokens(torch.randint(0, 900, (1, 20), generator=g).cuda())
    with pytest.raises(ValueError, match="fused"):
        tiny.generate(inputs_embeds=et, max_new_tokens=4, prompt_lookup_num_tokens=3)
    tiny.refuse()
    assert tiny.generate(inputs_embeds=et, max_new_tokens=4, eos_token_id=-1, prompt_lookup_num_tokens=3).shape == (1, 4)
    # a head dim other than 128
    tiny.lcfg.head_dim = 64
    try:
        with pytest.raises(ValueError, match="head_dim 128"):
            tiny.generate(inputs_embeds=et, max_new_tokens=4, prompt_lookup_num_tokens=3)
    finally:
        tiny.lcfg.head_dim = 128

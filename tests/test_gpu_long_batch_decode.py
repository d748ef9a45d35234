"""Batched decode past 2048 cached positions (bdec_attn_walk_kernel, vila_attn_decode_batch_bf16, the `_ctx` workspace sizes,
batch_open(max_ctx <= 32768)): beyond 2048 positions the attention's blocks walk chunks s, s + NSL, ... of a row with an online softmax.  The
kernel against an fp32 softmax, the rows of a long batch against their solo runs, continuous batching over a 4096-position cache, the W4 and
the sampled step, and what is refused."""
import ctypes as C
import zlib

import pytest
import torch

from tests.gpu_util import rel_l2
from vila_amd import _lib, configs, ops, synthetic
from vila_amd._lib import check

pytestmark = pytest.mark.gpu


def _8b():
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    return cfg


def _batch(llm, lens, seed, vocab=31000):
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.randint(0, vocab, (len(lens), L), generator=g)
    mask = torch.zeros(len(lens), L, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, :n] = True
    return llm.embed_tokens(ids.cuda()), mask.cuda()


class _Slices:
    """vila_decode_batch_force_slices for a `with` block; always back to automatic."""

    def __init__(self, nsl):
        self.nsl = nsl

    def __enter__(self):
        _lib.load().vila_decode_batch_force_slices(int(self.nsl))

    def __exit__(self, *a):
        _lib.load().vila_decode_batch_force_slices(0)


# ---- 1. the kernel against fp32 -------------------------------------------------------------------------------------------------------
MAX_CTX, KV = 4096, 2
# rows of one launch: short and long side by side; together the eight lengths of the issue (a block with no chunk, a chunk with one key,
# slices walking 2 / 2 / 2 and 6 / 5 / 5 chunks under force_slices(3), a capacity-full row)
LAUNCHES = [(1, 4096, 257), (255, 1536, 2049), (256, 769, 4096)]


@pytest.fixture(scope="module")
def kv_cache():
    g = torch.Generator().manual_seed(5)
    k = torch.randn((3, KV, MAX_CTX, 128), generator=g).to(torch.bfloat16).cuda()
    v = torch.randn((3, KV, MAX_CTX, 128), generator=g).to(torch.bfloat16).cuda()
    return k, v


def _ref(q, k, v, lens, scale):
    n, nq, _ = q.shape
    G = nq // KV
    out = torch.empty((n, nq, 128), dtype=torch.float32, device=q.device)
    for i, L in enumerate(lens):
        kk = k[i, :, :L].float().repeat_interleave(G, 0)                 # [nq, L, 128]
        vv = v[i, :, :L].float().repeat_interleave(G, 0)
        s = torch.einsum("hd,hld->hl", q[i].float(), kk) * scale
        out[i] = torch.einsum("hl,hld->hd", torch.softmax(s, -1), vv)
    return out


@pytest.mark.parametrize("G", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("force", [0, 16, 3])
def test_walking_attention_against_fp32_softmax(kv_cache, G, force):
    """max|o - ref| <= 2^-7 max|V|: the output is a convex combination of V rounded once to bf16 (relative 2^-9); the factor 4 covers __expf and
    the summation order.  force 0: the automatic count (8 slices: up to 2 chunks per block); 16: one chunk per block at most; 3: slices walk up to 6
    chunks."""
    k, v = kv_cache
    scale = 128 ** -0.5
    g = torch.Generator().manual_seed(100 + G)
    bound = 2.0 ** -7 * float(v.float().abs().max())
    try:
        _lib.load().vila_decode_batch_force_slices(force)
        for lens in LAUNCHES:
            q = torch.randn((3, KV * G, 128), generator=g).to(torch.bfloat16).cuda()
            pos = torch.tensor([L - 1 for L in lens], dtype=torch.int32, device="cuda")
            o = ops.attn_decode_batch(q, k, v, pos, scale)
            torch.cuda.synchronize()
            ref = _ref(q, k, v, lens, scale)
            for i, L in enumerate(lens):
                err = float((o[i].float() - ref[i]).abs().max())
                print(f"G={G} force={force} keys={L}: max|o - ref| = {err:.3e} (bound {bound:.3e})")
                assert err <= bound, f"G={G} force={force} row of {L} keys: {err:.3e} > {bound:.3e}"
    finally:
        _lib.load().vila_decode_batch_force_slices(0)


# ---- 2. rows against solo runs ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_8b():
    from vila_amd.vlm import build_model
    return build_model(_8b(), seed=9)


@pytest.mark.parametrize("force", [0, 2])
def test_long_batch_rows_against_their_solo_runs(model_8b, force):
    """A padded batch of 2400 / 2100 / 300 keys takes the batched step in a cache of more than 2048 positions; every row's last-step logits
    against its solo teacher-forced run (the suite's decode tolerance) and its ids under the margin rule.  force 0: the automatic 8 slices (the two
    long rows walk 2 chunks in slices 0 and 1); force 2: the long rows walk 5 chunks per block.  The session (and its captured graph, which bakes the slice count) is dropped first, so
    each case captures its own steps."""
    llm = model_8b.llm
    n_new, tol = 4, 1.5e-2
    e, mask = _batch(llm, [2400, 2100, 300], 31)
    llm._drop_batch_session()
    with _Slices(force):
        out = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=-1)
        assert getattr(llm, "_bdecode", None) is not None, "the batched path was not taken"
        assert llm._bdecode.cache.max_ctx == 2560 and llm._bdecode.graph is not None
        assert llm._bdecode.attn_slices == (force or 8), f"the session's steps launch {llm._bdecode.attn_slices} slices"
        assert _lib.load().vila_decode_batch_slices(2560) == (force or 8)
        blog = llm._bdecode.logits.clone()
    llm._drop_batch_session()                                        # nothing later replays a graph captured under the hook
    assert out.shape == (3, n_new)
    for b in range(3):
        _, lg = llm.generate(inputs_embeds=e[b:b + 1], attention_mask=mask[b:b + 1], max_new_tokens=n_new, return_logits=True, use_graph=False,
                             eos_token_id=-1, forced_ids=out[b])
        rel = rel_l2(blog[b], lg[-1])
        print(f"force={force} row {b}: last-step logits rel_l2 = {rel:.3e}")
        assert rel < tol, f"row {b} ({int(mask[b].sum())} keys): step logits rel={rel:.3e}"
        ids, lgs = llm.generate(inputs_embeds=e[b:b + 1], attention_mask=mask[b:b + 1], max_new_tokens=n_new, return_logits=True, use_graph=False,
                                eos_token_id=-1)
        top2 = lgs.float().topk(2, -1).values
        margin = (top2[:, 0] - top2[:, 1]).cpu()
        bound = 4 * tol * float(lgs.float().abs().max())
        got, want = out[b].cpu(), ids[0].cpu()
        for t in range(n_new):
            if got[t] != want[t]:
                assert float(margin[t]) <= bound, f"row {b} step {t}: ids {got.tolist()} vs solo {want.tolist()} at a decisive step"
                break


# ---- 3. continuous batching over a long cache ------------------------------------------------------------------------------------------
def test_continuous_batching_over_a_4096_position_cache(model_8b):
    """batch_open(4, 4096, 16): a 2300-key row, 3 steps, a 40-key row joins another slot, 5 more; both rows equal their solo runs up to the first
    non-decisive step, and the graph replay equals eager launches from the same state."""
    llm = model_8b.llm
    llm._drop_batch_session()
    g = torch.Generator().manual_seed(41)
    lens = {"A": 2300, "B": 40}
    e = {k: llm.embed_tokens(torch.randint(0, 31000, (1, n), generator=g).cuda()) for k, n in lens.items()}
    steps = {"A": 8, "B": 5}
    solo = {}
    for k in lens:
        ids, lg = llm.generate(inputs_embeds=e[k], max_new_tokens=steps[k] + 1, return_logits=True, use_graph=False, eos_token_id=-1)
        top2 = lg.float().topk(2, -1).values
        solo[k] = (ids[0].cpu(), (top2[:, 0] - top2[:, 1]).cpu(), float(lg.float().abs().max()))
    st = llm.batch_open(4, 4096, 16)
    assert st.cache.max_ctx == 4096 and st.attn_slices == 8
    got = {"A": [llm.batch_admit(st, 0, e["A"][0])]}
    llm.batch_run(st, 3)
    got["B"] = [llm.batch_admit(st, 2, e["B"][0])]
    state = (st.pos.clone(), st.n_out.clone(), st.token.clone(), st.out_ids.clone())
    llm.batch_run(st, 5)
    n = st.n_out.tolist()
    assert n[0] == 8 and n[2] == 5
    got["A"] += st.out_ids[0, :8].tolist()
    got["B"] += st.out_ids[2, :5].tolist()
    for k, toks in got.items():
        want, margin, top = solo[k]
        bound = 4 * 1.5e-2 * top
        for t, (a, b) in enumerate(zip(toks, want.tolist())):
            if a != b:
                assert float(margin[t]) <= bound, f"row {k} step {t}: {toks} vs solo {want.tolist()} at a decisive step (margin {float(margin[t]):.3f})"
                break
    # the graph replay == eager launches of the step from the same state (the 5 steps re-write the same cache positions with the same values)
    replay = (st.out_ids.clone(), st.token.clone(), st.logits.clone())
    st.pos.copy_(state[0]); st.n_out.copy_(state[1]); st.token.copy_(state[2]); st.out_ids.copy_(state[3])
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(st.stream):
        for _ in range(5):
            llm._batch_step(st)
    st.stream.synchronize()
    assert torch.equal(st.out_ids, replay[0]) and torch.equal(st.token, replay[1]) and torch.equal(st.logits, replay[2])


# ---- 4. W4 and sampling ----------------------------------------------------------------------------------------------------------------
def _exact_w4(shape, seed, log2_scale):
    """Weights that int4 groups of 128 represent exactly (as tests/test_gpu_w4_batch_decode.py builds them)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-8, 8, shape, generator=g).float()
    e = torch.tensor(log2_scale, dtype=torch.float32)[torch.randint(0, len(log2_scale), (shape[0], shape[1] // 128), generator=g)]
    return (q.view(shape[0], -1, 128) * torch.exp2(e)[..., None]).view(shape)


def test_w4_batched_step_over_a_4096_position_cache():
    """The tiny head-dim-128 W4 model: a 2100-key row and a short one in a 4096-position session; the step's logits against the solo W4 step of
    each row, teacher-forced alike, at the W4 batched tests' tolerance (rel_l2 < 1.5e-2, _rows_vs_solo)."""
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152
    cfg.llm.max_position_embeddings = max(getattr(cfg.llm, "max_position_embeddings", 0) or 0, 4096)
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    for k in list(w):
        if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
            w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, (-7, -6, -5))
    model = build_model(cfg, weights=w)
    llm = model.llm
    llm.quantize_w4(batch_decode=True)
    lens = [2100, 33]
    e, mask = _batch(llm, lens, 7, vocab=900)
    st = llm.batch_open(2, 4096, 8)
    assert st.key[-1] == llm._w4.mats[0]["down"].q.data_ptr() and st.cache.max_ctx == 4096
    first = [llm.batch_admit(st, b, e[b, :n]) for b, n in enumerate(lens)]
    llm.batch_run(st, 2)
    blog = st.logits.clone()
    fed = [[first[b]] + st.out_ids[b, :2].tolist() for b in range(2)]
    for b, n in enumerate(lens):
        _, lg = llm.generate(inputs_embeds=e[b:b + 1, :n], max_new_tokens=3, return_logits=True, use_graph=False, eos_token_id=-1,
                             forced_ids=torch.tensor(fed[b]))
        rel = rel_l2(blog[b], lg[-1])
        print(f"W4 row of {n} keys: step logits rel_l2 = {rel:.3e}")
        assert rel < 1.5e-2, f"W4 row of {n} keys: rel={rel:.3e}"


def test_sampled_step_over_a_4096_position_cache(model_8b):
    """One greedy and one sampled row (0.2 / 50 / 0.9, fixed seed): the sampled token is bit-equal to ops.sample on that step's logits row with
    the same counter, the greedy row's token is the argmax."""
    llm = model_8b.llm
    lens = [2100, 60]
    e, _ = _batch(llm, lens, 53)
    st = llm.batch_open(2, 4096, 8, sampling=True)
    assert st.sampling and st.cache.max_ctx == 4096
    sp = (0.2, 50, 0.9, 1234)
    llm.batch_admit(st, 0, e[0, :lens[0]])
    llm.batch_admit(st, 1, e[1, :lens[1]], sampling=sp)
    llm.batch_run(st, 2)
    counter = (st.pos[1:2] - 1).to(torch.int32)                       # the position of the token the last step consumed
    want = ops.sample(st.logits[1], sp[0], sp[1], sp[2], sp[3], counter=counter)
    assert int(st.token[1]) == int(want), (int(st.token[1]), int(want))
    assert int(st.token[0]) == int(st.logits[0].argmax())


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_long_caches_need_the_ctx_workspace_and_short_sessions_keep_theirs(model_8b):
    llm = model_8b.llm
    lib = _lib.load()
    w = llm._struct()
    with pytest.raises(ValueError):
        llm.batch_open(4, 32769, 8)
    st = llm.batch_open(4, 4096, 8)
    small = lib.vila_llm_decode_batch_workspace_bytes(C.byref(w.shape), 4)
    assert lib.vila_llm_decode_batch_workspace_bytes_ctx(C.byref(w.shape), 4, 4096) > small
    assert lib.vila_llm_decode_batch_workspace_bytes_ctx(C.byref(w.shape), 4, 2048) == small
    assert lib.vila_llm_decode_batch_workspace_bytes_ctx(C.byref(w.shape), 4, 512) == small
    before = (st.pos.clone(), st.n_out.clone(), st.token.clone())
    with pytest.raises(ValueError, match="2048"):
        check(lib.vila_llm_decode_step_batch(C.byref(w), C.byref(st.cache.c), C.byref(st.c), st.ws.data_ptr(), small, None), "step")
    torch.cuda.synchronize()
    for a, b in zip(before, (st.pos, st.n_out, st.token)):
        assert torch.equal(a, b), "a refused step changed the batch state"
    # a short session with the workspace of the function without `_ctx`
    st = llm.batch_open(4, 512, 8)
    assert st.ws.numel() == small
    e, _ = _batch(llm, [20], 3)
    llm.batch_admit(st, 0, e[0])
    check(lib.vila_llm_decode_step_batch(C.byref(w), C.byref(st.cache.c), C.byref(st.c), st.ws.data_ptr(), small, None), "step")
    torch.cuda.synchronize()
    assert int(st.pos[0]) == 21 and int(st.n_out[0]) == 1

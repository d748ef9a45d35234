"""Batched decode over a shared prompt prefix on the GPU: vila_attn_decode_batch_prefix_bf16 (bdec_attn_shared_kernel<.., true>, bdec_attn_walk_kernel<.., true>,
bdec_attn_prefix_merge_kernel), the four vila_llm_decode_step_batch_prefix* steps, batch_open(shared_prefix=True) / batch_set_prefix / batch_admit(share=True)
and generate(num_return_sequences=)."""
import ctypes as C

import pytest
import torch

from tests.gpu_util import rel_l2
from vila_amd import _lib, configs, ops, synthetic

pytestmark = pytest.mark.gpu


class _Slices:
    """vila_decode_batch_force_slices for a `with` block; always back to automatic."""

    def __init__(self, nsl):
        self.nsl = nsl

    def __enter__(self):
        _lib.load().vila_decode_batch_force_slices(int(self.nsl))

    def __exit__(self, *a):
        _lib.load().vila_decode_batch_force_slices(0)


def _i32(x):
    return torch.tensor(list(x) if isinstance(x, (list, tuple)) else [x], dtype=torch.int32, device="cuda")


# ---- the operator ------------------------------------------------------------------------------------------------------------------------
MAX_CTX, KV, SLOTS = 4096, 2, 17          # 16 row slots and the prefix slot (the last)
PFX = SLOTS - 1


@pytest.fixture(scope="module")
def kv_cache():
    """One layer's cache [17][2][4096][128], random bf16.  Slots 3 and 15 hold slot 0's rows, so that one sequence can sit at three row indices."""
    g = torch.Generator().manual_seed(11)
    k = torch.randn((SLOTS, KV, MAX_CTX, 128), generator=g).to(torch.bfloat16)
    v = torch.randn((SLOTS, KV, MAX_CTX, 128), generator=g).to(torch.bfloat16)
    for s in (3, 15):
        k[s] = k[0]; v[s] = v[0]
    return k.cuda(), v.cuda()


def _reference(q, k, v, S, pos, uses, G, scale):
    """fp32 softmax attention of every row over the keys the semantics give it."""
    out = []
    for i, (p, u) in enumerate(zip(pos, uses)):
        if u and S > 0:
            kk = torch.cat([k[PFX, :, :S], k[i, :, S:p + 1]], 1).float()
            vv = torch.cat([v[PFX, :, :S], v[i, :, S:p + 1]], 1).float()
        else:
            kk, vv = k[i, :, :p + 1].float(), v[i, :, :p + 1].float()
        s = torch.einsum("hd,hld->hl", q[i].float(), kk.repeat_interleave(G, 0)) * scale
        out.append(torch.einsum("hl,hld->hd", torch.softmax(s, -1), vv.repeat_interleave(G, 0)))
    return torch.stack(out)


# (S, pos, uses): no prefix although every flag is set; one private key; the private chunk full; a second private chunk begins; the last position with
# 15 prefix chunks walked; an ordinary row below S between two sharers above it; a single row
CASES = [
    (0, [0, 300, 4095], [1, 1, 1]),
    (256, [256] * 3, [1, 1, 1]),
    (256, [511] * 3, [1, 1, 1]),
    (256, [512] * 3, [1, 1, 1]),
    (3840, [4095] * 3, [1, 1, 1]),
    (512, [700, 10, 900], [1, 0, 1]),
    (512, [700], [1]),
]
# n = 16: 112 columns at G = 7 (two column blocks, the second with a partial tile), 128 at G = 8; flags and positions mixed
POS16 = [700, 10, 900, 512, 4095, 767, 768, 0, 1300, 513, 2047, 2048, 255, 3000, 600, 1023]
USES16 = [1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("G", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("force", [0, 3])
def test_prefix_attention_against_fp32_softmax(kv_cache, G, force):
    """max|o - ref| <= 2^-7 max|V|: the bound and rationale of test_shared_attention_against_fp32_softmax (a convex combination of V rows rounded once to
    bf16, relative 2^-9, times 4 for __expf, the summation order and the prefix phase's bf16 P).  force 0: 8 slices in either phase; 3: up to 6 chunks each."""
    k, v = kv_cache
    scale = 128 ** -0.5
    g = torch.Generator().manual_seed(300 + G)
    bound = 2.0 ** -7 * float(v.float().abs().max())
    cases = CASES + ([(512, POS16, USES16)] if G in (7, 8) else [])
    with _Slices(force):
        for S, pos, uses in cases:
            n = len(pos)
            q = torch.randn((n, KV * G, 128), generator=g).to(torch.bfloat16).cuda()
            o = ops.attn_decode_batch_prefix(q, k, v, _i32(pos), _i32(S), _i32(uses), shared_len_host=S, scale=scale)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(o.float()).all()), f"G={G} force={force} S={S} pos={pos}: non-finite output"
            err = (o.float() - _reference(q, k, v, S, pos, uses, G, scale)).abs().amax((1, 2)).tolist()
            print(f"G={G} force={force} S={S} n={n}: max|o - ref| per row = {[f'{e:.2e}' for e in err]} (bound {bound:.3e})")
            for i, e in enumerate(err):
                assert e <= bound, f"G={G} force={force} S={S} row {i} (pos {pos[i]}, uses {uses[i]}): {e:.3e} > {bound:.3e}"


@pytest.mark.parametrize("force", [0, 3])
def test_prefix_attention_reads_only_its_keys(kv_cache, force):
    """NaN in every row the semantics say is never read — the prefix slot at or beyond S, a sharing row's own slot below S and above pos, an ordinary
    row's slot above pos — leaves the outputs finite and bit-equal to the clean run."""
    k, v = kv_cache
    S, pos, uses, G = 512, [700, 10, 900], [1, 0, 1], 7
    q = torch.randn((3, KV * G, 128), generator=torch.Generator().manual_seed(41)).to(torch.bfloat16).cuda()
    kp, vp = k.clone(), v.clone()
    for t in (kp, vp):
        t[PFX, :, S:] = float("nan")
        for i, (p, u) in enumerate(zip(pos, uses)):
            t[i, :, p + 1:] = float("nan")
            if u:
                t[i, :, :S] = float("nan")
    with _Slices(force):
        clean = ops.attn_decode_batch_prefix(q, k, v, _i32(pos), _i32(S), _i32(uses), shared_len_host=S)
        dirty = ops.attn_decode_batch_prefix(q, kp, vp, _i32(pos), _i32(S), _i32(uses), shared_len_host=S)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dirty.float()).all())
    assert torch.equal(clean, dirty)


def test_sharing_row_does_not_depend_on_the_batch(kv_cache):
    """Invariance (a): the sharing row at S = 512, pos = 700 gives the same bits alone, as row 3 of 5 and as row 15 of 16 at G = 7 (another column tile,
    the second column block) among rows whose flags and positions differ.  Slots 0, 3 and 15 of the fixture hold the same rows."""
    k, v = kv_cache
    G, S = 7, 512
    g = torch.Generator().manual_seed(78)
    q = torch.randn((16, KV * G, 128), generator=g).to(torch.bfloat16).cuda()
    row = q[0:1].clone()
    alone = ops.attn_decode_batch_prefix(row, k, v, _i32([700]), _i32(S), _i32([1]), shared_len_host=S)
    q5 = q[:5].clone(); q5[3] = row[0]
    mid = ops.attn_decode_batch_prefix(q5, k, v, _i32([900, 30, 512, 700, 2000]), _i32(S), _i32([1, 0, 1, 1, 0]), shared_len_host=S)
    q16 = q.clone(); q16[15] = row[0]
    pos16, uses16 = list(POS16), [1 - u for u in USES16]
    pos16[15], uses16[15] = 700, 1
    pos16 = [max(p, S) if u else p for p, u in zip(pos16, uses16)]
    full = ops.attn_decode_batch_prefix(q16, k, v, _i32(pos16), _i32(S), _i32(uses16), shared_len_host=S)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], mid[3]) and torch.equal(alone[0], full[15])


@pytest.mark.parametrize("force", [3, 0])
def test_ordinary_row_equals_the_batched_attention(kv_cache, force):
    """Invariance (b): the rows with uses = 0 of a prefix session equal ops.attn_decode_batch bit for bit under the same slice count (forced 3; 0: the
    automatic 8 of a 4096-position cache, where that operator walks too)."""
    k, v = kv_cache
    G, S = 7, 512
    q = torch.randn((16, KV * G, 128), generator=torch.Generator().manual_seed(79)).to(torch.bfloat16).cuda()
    with _Slices(force):
        o = ops.attn_decode_batch_prefix(q, k, v, _i32(POS16), _i32(S), _i32(USES16), shared_len_host=S)
        ref = ops.attn_decode_batch(q, k, v, _i32(POS16))
    torch.cuda.synchronize()
    plain = [i for i, u in enumerate(USES16) if not u]
    assert len(plain) >= 4
    for i in plain:
        assert torch.equal(o[i], ref[i]), f"row {i} (pos {POS16[i]})"
    assert not torch.equal(o[0], ref[0])                       # a sharing row reads other keys


def test_prefix_attention_refuses_bad_arguments(kv_cache):
    k, v = kv_cache
    q = torch.zeros((3, KV * 7, 128), dtype=torch.bfloat16, device="cuda")
    pos, uses = _i32([600, 600, 600]), _i32([1, 1, 1])
    with pytest.raises(ValueError, match="multiple of 256"):
        ops.attn_decode_batch_prefix(q, k, v, pos, _i32(300), uses, shared_len_host=300)
    with pytest.raises(ValueError, match="prefix slot"):
        ops.attn_decode_batch_prefix(q, k, v, pos, _i32(256), uses, prefix_slot=SLOTS, shared_len_host=256)
    with pytest.raises(ValueError, match="prefix slot"):
        ops.attn_decode_batch_prefix(q, k, v, pos, _i32(256), uses, prefix_slot=1, shared_len_host=256)
    with pytest.raises(ValueError, match="GQA group"):
        ops.attn_decode_batch_prefix(torch.zeros((3, KV * 3, 128), dtype=torch.bfloat16, device="cuda"), k, v, pos, _i32(256), uses, shared_len_host=256)


# ---- the step against solo runs ------------------------------------------------------------------------------------------------------------
def _8b():
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    return cfg


@pytest.fixture(scope="module")
def model_8b():
    from vila_amd.vlm import build_model
    return build_model(_8b(), seed=9)


def _rows_vs_solo(llm, vocab_hi, seed, tol=1.5e-2):
    """A prefix of 600 tokens (S = 512), three sharers whose prompts go on for 5, 40 and 300 tokens, one ordinary row of 300; 4 steps of the captured
    graph.  Every row's last-step logits against its solo teacher-forced run (rel_l2 < tol) and its ids under the margin rule (bound
    4 tol max|logit|), as test_long_batch_rows_against_their_solo_runs does them; then what the steps wrote."""
    g = torch.Generator().manual_seed(seed)
    ids = lambda n: torch.randint(0, vocab_hi, (n,), generator=g)
    pre = ids(600)
    prompts = [torch.cat([pre, ids(t)]) for t in (5, 40, 300)] + [ids(300)]
    shares = [True, True, True, False]
    emb = [llm.embed_tokens(p[None].cuda())[0] for p in prompts]
    n_steps = 4
    llm._drop_batch_session()
    st = llm.batch_open(4, 1024, 8, shared_prefix=True)
    assert st.cache.n_slots == 5 and st.prefix_slot == 4 and st.graph is not None
    S = llm.batch_set_prefix(st, llm.embed_tokens(pre[None].cuda())[0])
    assert S == 512 and int(st.shared_len) == 512
    pk, pv = st.cache.k[:, 4, :, :S].clone(), st.cache.v[:, 4, :, :S].clone()
    first = [llm.batch_admit(st, b, emb[b], share=shares[b]) for b in range(4)]
    assert st.uses.tolist() == [1, 1, 1, 0] and st.pos.tolist() == [len(p) for p in prompts]
    k0, v0 = st.cache.k.clone(), st.cache.v.clone()
    llm.batch_run(st, n_steps)
    assert st.n_out.tolist() == [n_steps] * 4
    blog = st.logits.clone()
    got_all = [[first[b]] + st.out_ids[b, :n_steps].tolist() for b in range(4)]
    k1, v1 = st.cache.k.clone(), st.cache.v.clone()
    llm._drop_batch_session()
    # the prefix slot's shared rows are untouched, and row b wrote rows P .. P + 3 of its own slot and nothing else
    for a, b_ in ((k0, k1), (v0, v1)):
        assert torch.equal(a[:, 4, :, :S], b_[:, 4, :, :S])
        assert torch.equal(b_[:, 4, :, :S], pk if a is k0 else pv), "an admission or a step wrote the shared rows of the prefix slot"
        for b in range(4):
            P = len(prompts[b])
            keep = torch.ones(1024, dtype=torch.bool, device="cuda"); keep[P:P + n_steps] = False
            assert torch.equal(a[:, b][:, :, keep], b_[:, b][:, :, keep]), f"row {b} wrote outside rows {P} .. {P + n_steps - 1} of its slot"
            assert not torch.equal(a[:, b, :, P:P + n_steps], b_[:, b, :, P:P + n_steps])
    for b in range(4):
        e, n_new = emb[b][None], n_steps + 1
        got = torch.tensor(got_all[b])
        _, lg = llm.generate(inputs_embeds=e, max_new_tokens=n_new, return_logits=True, use_graph=False, eos_token_id=-1, forced_ids=got.cuda())
        rel = rel_l2(blog[b], lg[-1])
        print(f"row {b} ({len(prompts[b])} keys, share={shares[b]}): last-step logits rel_l2 = {rel:.3e}")
        assert rel < tol, f"row {b}: step logits rel={rel:.3e}"
        sid, lgs = llm.generate(inputs_embeds=e, max_new_tokens=n_new, return_logits=True, use_graph=False, eos_token_id=-1)
        top2 = lgs.float().topk(2, -1).values
        margin = (top2[:, 0] - top2[:, 1]).cpu()
        bound = 4 * tol * float(lgs.float().abs().max())
        want = sid[0].cpu()
        for t in range(n_new):
            if got[t] != want[t]:
                assert float(margin[t]) <= bound, f"row {b} step {t}: ids {got.tolist()} vs solo {want.tolist()} at a decisive step"
                break


def test_prefix_step_rows_against_their_solo_runs(model_8b):
    _rows_vs_solo(model_8b.llm, 31000, 71)


def _exact_w4(shape, seed, log2_scale):
    """Weights that int4 groups of 128 represent exactly (as tests/test_gpu_w4_batch_decode.py builds them)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-8, 8, shape, generator=g).float()
    e = torch.tensor(log2_scale, dtype=torch.float32)[torch.randint(0, len(log2_scale), (shape[0], shape[1] // 128), generator=g)]
    return (q.view(shape[0], -1, 128) * torch.exp2(e)[..., None]).view(shape)


def test_prefix_step_rows_against_their_solo_runs_w4():
    """The same on configs.tiny with exact-int4 weights, built as test_verify_rows_against_solo_runs_w4 builds them."""
    import zlib
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    for k in list(w):
        if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
            w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, (-7, -6, -5))
    llm = build_model(cfg, weights=w).llm
    llm.quantize_w4(batch_decode=True)
    _rows_vs_solo(llm, 900, 72)


# ---- n samples of one prompt ---------------------------------------------------------------------------------------------------------------
def test_num_return_sequences_sampled(model_8b):
    """generate(num_return_sequences=4): [4, T]; row j's logits at every step within the decode tolerance of its own solo sampled run with seed
    seed + j, teacher-forced on row j's ids; the rows are not all equal; two calls give the same ids."""
    llm = model_8b.llm
    T, tol, seed = 4, 1.5e-2, 1234
    e = llm.embed_tokens(torch.randint(0, 31000, (1, 300), generator=torch.Generator().manual_seed(73)).cuda())
    kw = dict(inputs_embeds=e, max_new_tokens=T, do_sample=True, temperature=1.0, top_k=50, top_p=0.95, seed=seed, eos_token_id=-1)
    llm._drop_batch_session()
    ids, lg = llm.generate(**kw, batch_sample=True, num_return_sequences=4, return_logits=True)
    assert ids.shape == (4, T) and lg.shape[:2] == (T, 4)
    assert llm._bdecode.shared_prefix and llm._bdecode.S == 256
    a = llm.generate(**kw, batch_sample=True, num_return_sequences=4)
    b = llm.generate(**kw, batch_sample=True, num_return_sequences=4)
    assert a.shape == (4, T) and torch.equal(a, b) and torch.equal(a.cpu(), ids.cpu())
    assert len({tuple(r) for r in a.tolist()}) > 1, "rows with distinct seeds drew the same ids"
    llm._drop_batch_session()
    for j in range(4):
        _, ls = llm.generate(**{**kw, "seed": seed + j}, return_logits=True, use_graph=False, forced_ids=ids[j])
        for t in range(T):
            rel = rel_l2(lg[t, j], ls[t])
            print(f"row {j} step {t}: logits rel_l2 = {rel:.3e}")
            assert rel < tol, f"row {j} step {t}: rel={rel:.3e}"


# ---- what is refused, before any launch ----------------------------------------------------------------------------------------------------
def test_shared_prefix_refusals(model_8b):
    llm = model_8b.llm
    g = torch.Generator().manual_seed(74)
    e = llm.embed_tokens(torch.randint(0, 31000, (1, 600), generator=g).cuda())
    with pytest.raises(ValueError, match="do_sample"):
        llm.generate(inputs_embeds=e, max_new_tokens=4, num_return_sequences=4)
    with pytest.raises(ValueError, match="2..16"):
        llm.generate(inputs_embeds=e, max_new_tokens=4, num_return_sequences=17, do_sample=True, batch_sample=True)
    with pytest.raises(ValueError, match="padded batch"):
        llm.generate(inputs_embeds=e.expand(2, -1, -1), max_new_tokens=4, num_return_sequences=4, do_sample=True, batch_sample=True)
    # a prompt below one chunk shares nothing: return_logits is refused before any work, and the plain call runs n ordinary rows
    with pytest.raises(ValueError, match="at least 256"):
        llm.generate(inputs_embeds=e[:, :100], max_new_tokens=3, num_return_sequences=2, do_sample=True, batch_sample=True, return_logits=True)
    llm._drop_batch_session()
    out = llm.generate(inputs_embeds=e[:, :100], max_new_tokens=3, num_return_sequences=2, do_sample=True, batch_sample=True, seed=5, eos_token_id=-1)
    assert out.shape == (2, 3) and llm._bdecode.S == 0 and llm._bdecode.staged_len is None
    llm._drop_batch_session()
    st = llm.batch_open(2, 1024, 8)
    with pytest.raises(ValueError, match="shared_prefix"):
        llm.batch_admit(st, 0, e[0], share=True)
    with pytest.raises(ValueError, match="shared_prefix"):
        llm.batch_set_prefix(st, e[0])
    st = llm.batch_open(2, 1024, 8, shared_prefix=True)
    with pytest.raises(ValueError, match="batch_set_prefix"):
        llm.batch_admit(st, 0, e[0], share=True)                # no prefix yet
    assert llm.batch_set_prefix(st, e[0]) == 512
    with pytest.raises(ValueError, match="shorter than the shared prefix"):
        llm.batch_admit(st, 0, e[0, :500], share=True)          # P < S
    llm.batch_admit(st, 0, e[0], share=True)
    with pytest.raises(ValueError, match="still share"):
        llm.batch_set_prefix(st, e[0, :300])                    # a live sharer
    llm.batch_release(st, [0])
    assert llm.batch_set_prefix(st, e[0, :300]) == 256
    # the plain step's workspace handed to a prefix step
    lib, w = _lib.load(), llm._struct()
    plain = lib.vila_llm_decode_batch_workspace_bytes_ctx(C.byref(w.shape), st.pos.numel(), 1024)
    assert plain < st.ws.numel() == lib.vila_llm_decode_batch_prefix_workspace_bytes(C.byref(w.shape), st.pos.numel(), 1024)
    rc = lib.vila_llm_decode_step_batch_prefix(C.byref(w), C.byref(st.cache.c), C.byref(st.c), C.byref(st.px), st.ws.data_ptr(), plain, ops._stream())
    assert rc == -1 and b"vila_llm_decode_batch_prefix" in lib.vila_last_error()
    llm._drop_batch_session()

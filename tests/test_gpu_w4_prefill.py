"""GPU tests of the W4A16 prefill (BASELINE configs[4]): the int4 GEMM (vila_gemm_w4_bf16 / vila_gemm_w4_qkv_bf16),
the int4 LLM prefill (vila_llm_prefill_w4) and quantize_w4(prefill=True, release_bf16=True).

Truth is the fp32 dequantise-then-matmul of the SAME quantised weights (W4Matrix.dequantized, W4Weights.dequantized_state) run through
the CPU oracle.  The model-level cases use ordinary seeded weights, so quantisation really changes them: the hybrid of earlier rounds
(bf16 prefill, int4 decode) computes a different model, and the discrimination checks below show the tests tell the two apart.
"""
import zlib

import pytest
import torch

from oracle import vila_oracle as O
from tests.gpu_util import max_abs, rel_l2
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu

PREFILL_BOUND = 2e-2

# (N, K, kind): NVILA-8B and NVILA-Lite-3B projections; kind "qkv" = (q_heads, kv_heads, head_dim)
SHAPES_8B = [((28, 4, 128), 3584, "qkv"), (3584, 3584, "plain"), (18944, 3584, "gateup"), (3584, 18944, "plain")]
SHAPES_3B = [((16, 2, 128), 2048, "qkv"), (2048, 2048, "plain"), (11008, 2048, "gateup"), (2048, 11008, "plain")]
SHAPES = SHAPES_8B + SHAPES_3B
M_LIST = [1, 5, 16, 17, 154, 256, 769, 1027]

_mats = {}


def _mat(shape, K, kind):
    """Packed matrix of seeded N(0, 0.02) weights (cached per shape) + its fp32 dequantised form on the GPU (natural row order)."""
    from vila_amd.quant import W4Matrix, rope_interleave_rows
    key = (shape, K, kind)
    if key not in _mats:
        g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        if kind == "qkv":
            nq, nkv, hd = shape
            N = (nq + 2 * nkv) * hd
            w = torch.randn(N, K, generator=g) * 0.02
            perm = rope_interleave_rows(nq + nkv, nq + 2 * nkv, hd, device="cuda")
            mat = W4Matrix.pack(w.cuda(), row_perm=perm)
            ref = (mat.dequantized(),)
        elif kind == "gateup":
            N = shape
            mat = W4Matrix.pack((torch.randn(N, K, generator=g) * 0.02).cuda(), (torch.randn(N, K, generator=g) * 0.02).cuda())
            ref = mat.dequantized()
        else:
            N = shape
            mat = W4Matrix.pack((torch.randn(N, K, generator=g) * 0.02).cuda())
            ref = (mat.dequantized(),)
        bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).cuda()
        _mats.clear()                                     # one shape resident at a time (gate/up at 8B widths is 0.3 GB of fp32)
        _mats[key] = (mat, ref, bias)
    return _mats[key]


def _x(M, K, seed, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return (mean + torch.randn(M, K, generator=g)).to(torch.bfloat16).cuda()


def _run(mat, kind, shape, x, bias=None, residual=None):
    from vila_amd import ops
    return ops.gemm_w4(x, mat, bias=bias, residual=residual, heads=shape if kind == "qkv" else None)


def _reference(ref, kind, x, bias=None, residual=None):
    xf = x.float()
    if kind == "gateup":
        return torch.nn.functional.silu(xf @ ref[0].T) * (xf @ ref[1].T)
    y = xf @ ref[0].T
    if bias is not None:
        y = y + bias.float()
    if residual is not None:
        y = y + residual.float()
    return y


def _check(y, ref, roundings=1):
    r = rel_l2(y, ref)
    assert r < 5e-3, f"rel-L2 {r:.3e}"
    # max-abs within a bf16 rounding of the output per rounding step (gate/up rounds g, u and silu(g) before the product, a residual is
    # added to the rounded projection: two)
    ulp = 2.0 ** -8 * float(ref.abs().max())
    err = max_abs(y, ref)
    assert err <= roundings * ulp, f"max-abs {err:.3e} vs {roundings} bf16 ulp {ulp:.3e}"


@pytest.fixture(autouse=True)
def _fp32_reference():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the GEMM op against fp32 dequantise-then-matmul
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,kind", SHAPES, ids=[f"{k}-{s}x{K}" for s, K, k in SHAPES])
def test_gemm_w4_vs_dequantised_fp32(shape, K, kind):
    mat, ref, bias = _mat(shape, K, kind)
    for M in M_LIST:
        x = _x(M, K, M)
        if kind == "plain":
            y = _run(mat, kind, shape, x)
            _check(y, _reference(ref, kind, x))
            res = _x(M, mat.N, M + 1)
            y = _run(mat, kind, shape, x, bias=bias, residual=res)
            # the residual is added to the bf16-rounded projection (as gemv_w4 and the bf16 GEMM do): compare with that rounding applied
            yr = (_reference(ref, kind, x, bias=bias).to(torch.bfloat16).float() + res.float())
            _check(y, yr, 2)
        elif kind == "qkv":
            _check(_run(mat, kind, shape, x, bias=bias), _reference(ref, kind, x, bias=bias))
        else:
            _check(_run(mat, kind, shape, x), _reference(ref, kind, x), 2)


def test_gemm_w4_in_place_residual():
    """x += W h with y aliasing the residual (the prefill's o_proj / down_proj), on a K-sliced (M = 5) and an unsliced (M = 769) grid."""
    mat, ref, _ = _mat(3584, 3584, "plain")
    for M in (5, 769):
        h = _x(M, 3584, 7)
        x = _x(M, 3584, 8)
        want = (_reference(ref, "plain", h).to(torch.bfloat16).float() + x.float())
        from vila_amd import ops
        ops.gemm_w4(h, mat, residual=x, out=x)
        _check(x, want, 2)


def test_gemm_w4_large_offsets_cancel():
    """Every q = 15 with zero = 0 and activations with a large mean: the kernel computes sum x (128 + 15) on the matrix cores and must
    cancel the 128-offset exactly enough to leave 15 sum x * scale."""
    from vila_amd import ops
    from vila_amd.quant import W4Matrix
    N, K = 512, 3584
    g = torch.Generator().manual_seed(5)
    k = torch.randint(6, 10, (N, 1), generator=g).float()
    w = (15.0 * torch.exp2(-k)).expand(N, K).contiguous()            # one positive value per row: scale 2^-k, zero 0, q = 15 everywhere
    mat = W4Matrix.pack(w.cuda())
    wq, wsz = mat.logical
    assert bool((wq == -1).all()), "not every nibble is 15"
    assert bool((((wsz >> 16) & 0xFFFF) == 0x4300).all()), "zero point is not 0 (bf16 128.0)"
    for M in (1, 17, 769):
        x = _x(M, K, 100 + M, mean=3.0)
        y = ops.gemm_w4(x, mat)
        ref = x.float() @ mat.dequantized().T
        _check(y, ref)


def test_gemm_w4_rejects_bad_shapes():
    from vila_amd import _lib, ops
    from vila_amd.quant import W4Matrix
    mat = W4Matrix.pack(torch.zeros((32, 256), device="cuda"))
    x = torch.zeros((4, 192), device="cuda", dtype=torch.bfloat16)
    lib = _lib.load()
    y = torch.zeros((4, 32), device="cuda", dtype=torch.bfloat16)
    # K not a multiple of the 128-wide group, N not a multiple of the 16-row tile, an unknown mode: -1 from the C ABI, ValueError above it
    assert lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), None, None, y.data_ptr(), 4, 32, 192, 0, None, 0, 0) == -1
    assert "multiple of the 128" in lib.vila_last_error().decode()
    assert lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), None, None, y.data_ptr(), 4, 24, 256, 0, None, 0, 0) == -1
    assert "multiple of the 16" in lib.vila_last_error().decode()
    assert lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), None, None, y.data_ptr(), 4, 32, 256, 3, None, 0, 0) == -1
    mat.K = 192
    with pytest.raises(ValueError, match="multiple of the 128"):
        ops.gemm_w4(x, mat)


@pytest.mark.parametrize("N,kind", [(16, "plain"), (48, "plain"), (1040, "plain"), (16, "gateup"), (1040, "gateup"), ((2, 1, 16), "qkv"),
                                    ((6, 2, 80), "qkv")])
def test_gemm_w4_partial_column_blocks(N, kind):
    """N not a multiple of the 128-row block: waves whose weight tiles lie past the end load nothing and write nothing."""
    K = 384
    mat, ref, bias = _mat(N, K, kind)
    for M in (1, 70, 769):
        x = _x(M, K, 40 + M)
        if kind == "plain":
            res = _x(M, mat.N, M + 2)
            y = _run(mat, kind, N, x, bias=bias, residual=res)
            _check(y, _reference(ref, kind, x, bias=bias).to(torch.bfloat16).float() + res.float(), 2)
        elif kind == "qkv":
            _check(_run(mat, kind, N, x, bias=bias), _reference(ref, kind, x, bias=bias))
        else:
            _check(_run(mat, kind, N, x), _reference(ref, kind, x), 2)


def test_gemm_w4_rejects_operands_the_mode_does_not_take():
    from vila_amd import _lib, ops
    mat, _, bias = _mat(64, 256, "gateup")
    x = _x(4, 256, 1)
    y = torch.zeros((4, 64), device="cuda", dtype=torch.bfloat16)
    lib = _lib.load()
    # gate/up takes neither a bias nor a residual
    assert lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), bias.data_ptr(), None, y.data_ptr(), 4, 64, 256, 1, None, 0, 0) == -1
    assert lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), None, y.data_ptr(), y.data_ptr(), 4, 64, 256, 1, None, 0, 0) == -1
    with pytest.raises(ValueError, match="bias"):
        ops.gemm_w4(x, mat, bias=bias)
    # head geometry that does not describe the matrix, a K that does not match x
    qmat, _, _ = _mat((2, 1, 16), 256, "qkv")
    with pytest.raises(ValueError, match="q\\|k\\|v rows"):
        ops.gemm_w4(x, qmat, heads=(2, 2, 16))
    with pytest.raises(ValueError, match="columns"):
        ops.gemm_w4(_x(4, 128, 1), qmat, heads=(2, 1, 16))


@pytest.mark.parametrize("M", [5, 769])
def test_gemm_w4_deterministic(M):
    """K-sliced (M = 5: fp32 slices added in a fixed order) and unsliced grids give bit-identical results from run to run."""
    for shape, K, kind in [(3584, 18944, "plain"), (18944, 3584, "gateup"), ((28, 4, 128), 3584, "qkv")]:
        mat, _, bias = _mat(shape, K, kind)
        x = _x(M, K, 31)
        a = _run(mat, kind, shape, x, bias=bias if kind == "qkv" else None)
        b = _run(mat, kind, shape, x, bias=bias if kind == "qkv" else None)
        assert torch.equal(a, b), kind


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the same math as the bf16 GEMM where int4 is exact
# ---------------------------------------------------------------------------------------------------------------------------------------
def _exact_w4(shape, seed, log2_scale=(-9, -8, -7)):
    """Weights exactly representable as (q - zero) * 2^k with every group spanning q = 0..15 (quantise -> dequantise is the identity)."""
    N, K = shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 16, (N, K // 128, 128), generator=g)
    q[..., 0], q[..., 1] = 0, 15
    zero = torch.randint(4, 12, (N, K // 128, 1), generator=g)
    k = torch.tensor(log2_scale)[torch.randint(0, len(log2_scale), (N, K // 128, 1), generator=g)]
    return ((q - zero).float() * torch.exp2(k.float())).view(N, K)


@pytest.mark.parametrize("N,K,M", [(3584, 3584, 769), (3584, 18944, 17), (2048, 11008, 154), (4608, 3584, 1)])
def test_gemm_w4_matches_bf16_gemm_on_exact_weights(N, K, M):
    from vila_amd import ops
    from vila_amd.quant import W4Matrix
    w = _exact_w4((N, K), N + K)
    mat = W4Matrix.pack(w.cuda())
    assert torch.equal(mat.dequantized().cpu(), w)
    x = _x(M, K, 3)
    y4 = ops.gemm_w4(x, mat)
    yb = ops.gemm(x, w.to(torch.bfloat16).cuda())
    assert rel_l2(y4, yb) < 2e-3, rel_l2(y4, yb)
    # gate/up rounds like gemv_w4 mode 1 (HF order: gate, up and silu(gate) in bf16 before the product), not like the fused bf16 EPI_GATEUP
    # (fp32 silu(g) * u): the bf16 comparison is the unfused route, two bf16 GEMMs and the activation on bf16 tensors
    wu = _exact_w4((N, K), N + K + 1)
    mat2 = W4Matrix.pack(w.cuda(), wu.cuda())
    y4 = ops.gemm_w4(x, mat2)
    yb = torch.nn.functional.silu(ops.gemm(x, w.to(torch.bfloat16).cuda())) * ops.gemm(x, wu.to(torch.bfloat16).cuda())
    assert rel_l2(y4, yb) < 2e-3, rel_l2(y4, yb)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3 - 7. the LLM prefill on the int4 weights
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cfg(name):
    if name == "tiny":
        cfg = configs.tiny("mlp_downsample")
        cfg.llm.intermediate_size = 1152                 # K of down_proj must be a multiple of the 128-wide group
        return cfg
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    return cfg


_models = {}


def _model(name, seed=3):
    """(bf16 weights, model quantised with prefill=True, oracle weights = the dequantised int4 projections + everything else bf16)."""
    from vila_amd.vlm import build_model
    if name not in _models:
        cfg = _cfg(name)
        w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, seed).items()}
        model = build_model(cfg, weights=w)
        q = model.llm.quantize_w4(prefill=True)
        wq = dict(w)
        wq.update(q.dequantized_state(model.llm))
        _models.clear()
        _models[name] = (cfg, w, model, wq)
    return _models[name]


def _embeds(cfg, w, T, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, min(cfg.image_token_id, cfg.llm.eos_token_id) - 1, (T,), generator=g)
    return w["llm.model.embed_tokens.weight"][ids].to(torch.bfloat16)


PROMPTS = {"single769": [769], "one": [1], "twelve": [12], "packed3": [300, 45, 424], "s2_2817": [2817]}


def _prefill_case(name, lens):
    cfg, w, model, wq = _model(name)
    llm = model.llm
    seqs = [_embeds(cfg, w, n, 17 + i) for i, n in enumerate(lens)]
    packed = torch.cat(seqs).cuda()
    T = packed.shape[0]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).cuda()
    seq = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(lens)]).cuda()
    cache = llm.new_cache(((max(lens) + 255) // 256) * 256, n_slots=len(lens))
    r = llm.prefill_packed(packed, pos, cu, max(lens), cache=cache, seq_of_tok=seq, want_all_logits=True)
    torch.cuda.synchronize()
    return cfg, w, model, wq, seqs, r.all_logits, cache


@pytest.mark.parametrize("name,prompt", [("tiny", p) for p in PROMPTS] + [("8b", p) for p in ("single769", "twelve", "packed3")])
def test_prefill_w4_vs_oracle(name, prompt):
    lens = PROMPTS[prompt]
    cfg, w, model, wq, seqs, lg, cache = _prefill_case(name, lens)
    lc = cfg.llm
    ref_logits = []
    for i, (e, n) in enumerate(zip(seqs, lens)):
        lo, past = O.qwen2_forward(e.float()[None], wq, lc)
        ref_logits.append(lo[0])
        # the KV cache: slot i, positions 0..n-1, every layer (RoPE applied to K, as the oracle's past holds it)
        for l in range(lc.num_hidden_layers):
            k_ref, v_ref = past[l][0][0], past[l][1][0]              # [kv_heads, n, hd]
            k_got = cache.k[l, i, :, :n].float().cpu()
            v_got = cache.v[l, i, :, :n].float().cpu()
            assert rel_l2(k_got, k_ref) < PREFILL_BOUND, (l, i, rel_l2(k_got, k_ref))
            assert rel_l2(v_got, v_ref) < PREFILL_BOUND, (l, i, rel_l2(v_got, v_ref))
    ref = torch.cat(ref_logits)
    err = rel_l2(lg, ref)
    assert err < PREFILL_BOUND, f"W4 prefill logits rel-L2 {err:.3e}"
    # discrimination: the bf16 prefill of the hybrid (quantize_w4() default) computes another model, far outside the bound
    llm = model.llm
    llm._w4_prefill = False
    try:
        packed = torch.cat(seqs).cuda()
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
        pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).cuda()
        hyb = llm.prefill_packed(packed, pos, cu, max(lens), want_all_logits=True).all_logits
    finally:
        llm._w4_prefill = True
    hyb_err = rel_l2(hyb, ref)
    assert hyb_err > 5 * PREFILL_BOUND, f"the hybrid's bf16 prefill is only {hyb_err:.3e} from the int4 oracle: the test cannot tell them apart"


@pytest.mark.parametrize("name", ["tiny", "8b"])
@pytest.mark.parametrize("T", [12, 769])
def test_prefill_w4_pruned_matches_full(name, T):
    """The generation prefill (last_rows: last layer's o_proj / MLP as W4 GEMVs for the one row) against the all-logits prefill's last row."""
    cfg, w, model, wq = _model(name)
    llm = model.llm
    e = _embeds(cfg, w, T, 5).cuda()
    pos = torch.arange(T, dtype=torch.int32, device="cuda")
    cache = llm.new_cache(((T + 255) // 256) * 256)
    last = torch.full((1,), T - 1, dtype=torch.int32, device="cuda")
    pruned = llm.prefill_packed(e, pos, None, T, cache=cache, last_rows=last).last_logits[0]
    full = llm.prefill_packed(e, pos, None, T, cache=llm.new_cache(((T + 255) // 256) * 256), want_all_logits=True).all_logits[T - 1]
    assert rel_l2(pruned, full) < 5e-3, rel_l2(pruned, full)


@pytest.mark.parametrize("name,T", [("tiny", 12), ("8b", 154)])
def test_generate_w4_prefill_vs_oracle(name, T):
    cfg, w, model, wq = _model(name)
    llm = model.llm
    n = 6
    e = _embeds(cfg, w, T, 9)
    ids_o, lg_o = O.greedy_generate(e.float()[None], wq, cfg, n, stop_at_eos=False)
    out, lg = llm.generate(inputs_embeds=e[None].cuda(), max_new_tokens=n, return_logits=True, forced_ids=ids_o, use_graph=False)
    err = max_abs(lg, lg_o)
    top2 = lg_o.topk(2, -1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 4 * err
    assert rel_l2(lg, lg_o) < 3e-2, f"W4 generate logits rel-L2 {rel_l2(lg, lg_o):.3e}"
    assert torch.equal(out[0].cpu()[decisive], ids_o[decisive])
    free_e = llm.generate(inputs_embeds=e[None].cuda(), max_new_tokens=n, use_graph=False, eos_token_id=-1)
    free_g = llm.generate(inputs_embeds=e[None].cuda(), max_new_tokens=n, use_graph=True, eos_token_id=-1)
    assert torch.equal(free_e, free_g)
    s1 = llm.generate(inputs_embeds=e[None].cuda(), max_new_tokens=n, do_sample=True, temperature=0.8, top_k=20, seed=1234, eos_token_id=-1)
    s2 = llm.generate(inputs_embeds=e[None].cuda(), max_new_tokens=n, do_sample=True, temperature=0.8, top_k=20, seed=1234, eos_token_id=-1)
    assert s1.shape == (1, n) and torch.equal(s1, s2)


def test_hf_forward_runs_w4_prefill():
    """The HF-style forward (inference logits) goes through the int4 prefill too."""
    cfg, w, model, wq = _model("tiny")
    e = _embeds(cfg, w, 20, 4)
    lg = model.llm(inputs_embeds=e[None].cuda()).logits[0]
    ref, _ = O.qwen2_forward(e.float()[None], wq, cfg.llm)
    assert rel_l2(lg, ref[0]) < PREFILL_BOUND


def test_default_quantize_keeps_bf16_prefill():
    """quantize_w4() with its defaults changes nothing about the prefill: first-token logits bit-equal to the un-quantised model's."""
    from vila_amd.vlm import build_model
    cfg = _cfg("tiny")
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    model = build_model(cfg, weights=w)
    e = _embeds(cfg, w, 40, 2).cuda()
    pos = torch.arange(40, dtype=torch.int32, device="cuda")
    last = torch.full((1,), 39, dtype=torch.int32, device="cuda")
    before = model.llm.prefill_packed(e, pos, None, 40, cache=model.llm.new_cache(256), last_rows=last).last_logits.clone()
    model.llm.quantize_w4()
    after = model.llm.prefill_packed(e, pos, None, 40, cache=model.llm.new_cache(256), last_rows=last).last_logits
    assert torch.equal(before, after)


def test_release_bf16_frees_projections_and_refuses_bf16_consumers(tmp_path):
    from vila_amd import checkpoint
    from vila_amd.train import FlatParams
    from vila_amd.vlm import build_model
    cfg = _cfg("8b")
    _models.clear()
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    model = build_model(cfg, weights=w)
    llm = model.llm
    with pytest.raises(ValueError, match="prefill=True"):
        llm.quantize_w4(release_bf16=True)
    llm.quantize_w4(keep_logical=False, prefill=True)
    e = _embeds(cfg, w, 100, 6)[None].cuda()
    ids_before = llm.generate(inputs_embeds=e, max_new_tokens=8, eos_token_id=-1)
    proj_bytes = sum(_proj.numel() * 2 for n, _proj in llm.named_parameters() if n.endswith("_proj.weight"))
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    freed = llm.release_bf16_projections()
    torch.cuda.synchronize()
    m1 = torch.cuda.memory_allocated()
    assert freed == proj_bytes
    assert m0 - m1 >= 0.9 * proj_bytes, (m0 - m1, proj_bytes)
    ids_after = llm.generate(inputs_embeds=e, max_new_tokens=8, eos_token_id=-1)
    assert torch.equal(ids_before, ids_after)
    # every consumer of the bf16 projections refuses, naming release_bf16
    pos = torch.arange(100, dtype=torch.int32, device="cuda")
    llm._w4_prefill = False
    try:
        with pytest.raises(RuntimeError, match="release_bf16"):
            llm.prefill_packed(e[0], pos, None, 100, want_all_logits=True)
    finally:
        llm._w4_prefill = True
    cache = llm.new_cache(256)
    st = llm._decode_session(cache, 4)
    w4 = llm._w4
    llm._w4 = None
    try:
        with pytest.raises(RuntimeError, match="release_bf16"):
            llm.decode_step(cache, st)
    finally:
        llm._w4 = w4
    with pytest.raises(RuntimeError, match="release_bf16"):
        llm.batch_open(2, 256, 8)
    with pytest.raises(RuntimeError, match="release_bf16"):
        llm._batch_session(2, 256, 8)
    with pytest.raises(RuntimeError, match="release_bf16"):
        FlatParams(model)
    with pytest.raises(RuntimeError, match="release_bf16"):
        checkpoint.save_pretrained(model, str(tmp_path / "ckpt"))
    with pytest.raises(RuntimeError, match="release_bf16"):
        llm.quantize_w4()
    # the released parameters are empty tensors: torch-level reads see no data (nothing points at freed memory)
    proj = [p for n, p in llm.named_parameters() if n.endswith("_proj.weight")]
    assert all(p.numel() == 0 and p.untyped_storage().nbytes() == 0 for p in proj)
    assert torch.cat([p.clone() for p in proj[:3]]).numel() == 0
    # loading weights, re-fusing and moving / converting refuse; a conversion that changes nothing leaves the model as it was
    with pytest.raises(RuntimeError, match="release_bf16"):
        model.load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError, match="release_bf16"):
        model.load_weights(w)
    with pytest.raises(RuntimeError, match="release_bf16"):
        llm.refuse()
    with pytest.raises(RuntimeError, match="release_bf16"):
        llm.to(torch.float16)
    with pytest.raises(RuntimeError, match="release_bf16"):
        model.to("cpu")
    assert model.cuda() is model and llm.to("cuda", torch.bfloat16) is llm
    assert torch.equal(llm.generate(inputs_embeds=e, max_new_tokens=8, eos_token_id=-1), ids_before)


def test_quantize_w4_release_in_one_call():
    """quantize_w4(prefill=True, release_bf16=True) on the tiny model: runs from int4 alone, and the oracle agrees."""
    from vila_amd.vlm import build_model
    cfg = _cfg("tiny")
    _models.clear()
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 3).items()}
    model = build_model(cfg, weights=w)
    q = model.llm.quantize_w4(prefill=True, release_bf16=True)
    wq = dict(w)
    wq.update(q.dequantized_state(model.llm))
    assert all(p.untyped_storage().nbytes() == 0 for n, p in model.llm.named_parameters() if n.endswith("_proj.weight"))
    e = _embeds(cfg, w, 30, 8)
    lg = model.llm(inputs_embeds=e[None].cuda()).logits[0]
    ref, _ = O.qwen2_forward(e.float()[None], wq, cfg.llm)
    assert rel_l2(lg, ref[0]) < PREFILL_BOUND

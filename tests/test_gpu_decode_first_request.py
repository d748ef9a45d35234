"""The batch-1 decode kernels take what their first memory requests need as flat leading arguments (preloaded into SGPRs at wave start), the CU
map as a few ints planned on the host (gemv_plan.h) and everything else as a by-value struct fetched behind the first requests (DESIGN.md §4.3,
"the head of a kernel").  What that can break: an argument that arrives in the wrong slot or by the wrong route, a map that differs from the
one the kernels used to derive, a tail field read before it is there.  So, with the arithmetic unchanged:

* every mode of `gemv_kernel` through `ops.gemv` (mode 0 plain / with norm / with bias and residual / fp32 output; mode 1 gate/up) and, for the
  merge mode 2, through `vila_attn_decode_oproj_bf16` (`ops.attn_decode(form="slices256", w=...)`), at N = 8 CUs + 2 and 8 CUs + 3 (the CU map; an
  odd last row), N = 1000 and N = 7 (the small grid) and K in {128, 3584, 18944, 18952} where the mode allows it (the merge needs whole heads:
  128, 3584 and 18944 = 148 heads), against the fp32 product at 4e-3 rel-L2 — the bias + residual bound of tests/test_gpu_decode_prologue_order.py,
  i.e. one bf16 rounding of the output — and with every row bit-equal between the CU-map grid and the small grids;
* attention + o_proj on 4 and 1 kv heads (G = 7 / 1) at positions 0, 255, 256 and 511 of a 512-position cache, read back through an identity
  o_proj weight, against `decode_attn_ref` at its bound (max|o - ref| <= 2^-7 max|V|, tests/test_decode_probe_cpu.py bound_of);
* the QKV + attention + o_proj chain inside a one-layer decode step (`qkv_decode_kernel` has no entry point of its own in the C ABI): 28 query
  heads on 4 kv heads at hidden 3584 (2304 row groups: the CU map; lm_head over K = 3584 keeps the struct head) and 1 on 1 at hidden 4096 (QKV
  on the small grid; lm_head over K = 4096 and 4100 rows takes the flat head on the CU map WITH the fused pick, `amax_v`, which `ops.gemv` does
  not reach), at positions 0, 255, 256 and 511 of a 512-position cache.  The K / V row the step writes is compared with the fp32 projection put
  through the kernel's roundings (bias, then HF's RoPE with bf16 cos / sin) at 4e-3 — one bf16 rounding, as above; the logits with an fp32
  reference of the whole layer (`decode_attn_ref` over the cache, every tensor rounded where the kernels round) at 2e-2, the bound the suite puts
  on a model's logits against the oracle (a chain of bf16 tensors: a rounding that falls the other way moves an element by 2^-8); the token
  must be the argmax of the logits;
* a solo step run twice from the same state at position 10 of a 1024-position session: identical logits bits, identical token, the token the
  argmax of the logits, and the K/V row the step wrote identical."""
import functools

import pytest
import torch

from tests.gpu_util import decode_attn_ref, randn_bf16, rel_l2, visible_upto
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu

BOUND = 4e-3          # tests/test_gpu_decode_prologue_order.py: one bf16 rounding of the output


@pytest.fixture(scope="module")
def ops():
    from vila_amd import ops as _ops
    return _ops


def _cus() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _ns():
    big = 8 * _cus() + 2
    assert big > 1000
    return [big + 1, big, 1000, 7]          # the widest first: the others are its leading rows


@functools.lru_cache(maxsize=2)
def _operands(K):
    """x, gain, W (8 CUs + 3 rows), W2, bias, residual and the fp32 products W x, W xn, W2 x, W2 xn — computed once per K."""
    N = _ns()[0]
    x = randn_bf16(K, seed=401)
    g = randn_bf16(K, seed=402, scale=0.1) + 1
    w = randn_bf16(N, K, seed=403, scale=K ** -0.5)
    w2 = randn_bf16(N, K, seed=404, scale=K ** -0.5)
    b, r = randn_bf16(N, seed=405), randn_bf16(N, seed=406)
    x32 = x.float()
    xn = (g * (x32 * torch.rsqrt(x32.pow(2).mean() + 1e-6)).to(torch.bfloat16)).float()      # HF's rounding order (tests/test_gpu_ops.py)
    return dict(x=x, g=g, w=w, w2=w2, b=b, r=r, wx=w.float() @ x32, wxn=w.float() @ xn, w2x=w2.float() @ x32, w2xn=w2.float() @ xn)


def _check_rows(what, outs, refs):
    """outs[N] against refs[:N] at BOUND; every N's rows bit-equal to the leading rows of the widest."""
    ns = sorted(outs, reverse=True)
    for n in ns:
        assert bool(torch.isfinite(outs[n].float()).all()), f"{what} N={n}: non-finite output"
        e = rel_l2(outs[n], refs[:n])
        print(f"{what} N={n}: rel={e:.3e}")
        assert e < BOUND, f"{what} N={n}: rel={e:.3e}"
    for n in ns[1:]:
        assert torch.equal(_bits(outs[n]), _bits(outs[ns[0]][:n])), f"{what}: rows of N={n} differ from the same rows of N={ns[0]}"


@pytest.mark.parametrize("K", [128, 3584, 18944, 18952])
def test_plain_gemv_every_epilogue(ops, K):
    d = _operands(K)
    bf = lambda t: t.to(torch.bfloat16).float()
    variants = {
        "plain": (dict(), bf(d["wx"])),
        "fp32 out": (dict(out_f32=True), d["wx"]),
        "norm": (dict(norm_w=d["g"], eps=1e-6), bf(d["wxn"])),
        "norm, fp32 out": (dict(norm_w=d["g"], eps=1e-6, out_f32=True), d["wxn"]),
        "bias": (dict(bias=d["b"]), bf(d["wx"] + d["b"].float())),
        "bias + residual": (dict(bias=d["b"], residual=d["r"]), bf(bf(d["wx"] + d["b"].float()) + d["r"].float())),
        "norm + residual": (dict(norm_w=d["g"], eps=1e-6, residual=d["r"]), bf(bf(d["wxn"]) + d["r"].float())),
    }
    for name, (kw, ref) in variants.items():
        outs = {}
        for n in _ns():
            kk = {k: (v[:n].contiguous() if k in ("bias", "residual") else v) for k, v in kw.items()}
            outs[n] = ops.gemv(d["x"], d["w"][:n], **kk)
        _check_rows(f"mode 0 {name} K={K}", outs, ref)


@pytest.mark.parametrize("K", [128, 3584, 18944, 18952])
def test_gate_up_gemv(ops, K):
    """HF: act(gate) * up with every tensor rounded to bf16 — the fp32 products through that chain of roundings."""
    d = _operands(K)
    bf = lambda t: t.to(torch.bfloat16).float()
    for name, kw, gk, uk in (("plain", dict(), "wx", "w2x"), ("norm", dict(norm_w=d["g"], eps=1e-6), "wxn", "w2xn")):
        ref = bf(bf(torch.nn.functional.silu(bf(d[gk]))) * bf(d[uk]))
        outs = {n: ops.gemv(d["x"], d["w"][:n], w2=d["w2"][:n], **kw) for n in _ns()}
        _check_rows(f"mode 1 {name} K={K}", outs, ref)


@functools.lru_cache(maxsize=None)
def _attn_operands(nq, nkv, cap):
    return randn_bf16(nq, 128, seed=411), randn_bf16(nkv, cap, 128, seed=412 + nq), randn_bf16(nkv, cap, 128, seed=413 + nq)


@pytest.mark.parametrize("nq,nkv", [(1, 1), (28, 4), (148, 37)])
def test_merge_gemv_through_attention_and_oproj(ops, nq, nkv):
    """Mode 2: x is the merge of the attention partials.  The reference is the fp32 softmax over the visible keys, rounded to bf16 as the kernel
    rounds its merged o, times W in fp32, plus the residual."""
    cap, K = 512, nq * 128
    q, k, v = _attn_operands(nq, nkv, cap)
    N = _ns()[0]
    w = randn_bf16(N, K, seed=414, scale=K ** -0.5)
    r = randn_bf16(N, seed=415)
    for p in (300,) if nq == 148 else (10, 300, 511):
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        o = decode_attn_ref(q[None], k[None], v[None], visible_upto([p + 1], cap, device="cuda"))[0]
        ref = ((w.float() @ o.to(torch.bfloat16).float().reshape(-1)).to(torch.bfloat16).float() + r.float()).to(torch.bfloat16).float()
        outs = {n: ops.attn_decode(q, k, v, pos, form="slices256", w=w[:n], residual=r[:n].contiguous()) for n in _ns()}
        _check_rows(f"mode 2 heads={nq} pos={p}", outs, ref)


@pytest.mark.parametrize("nq,nkv", [(28, 4), (1, 1)])
def test_attention_oproj_chain_against_the_softmax_reference(ops, nq, nkv):
    cap, K = 512, nq * 128
    q, k, v = _attn_operands(nq, nkv, cap)
    eye = torch.eye(K, dtype=torch.bfloat16, device="cuda")                       # y = o, bit for bit
    bound = 2.0 ** -7 * float(v.float().abs().max())
    for p in (0, 255, 256, cap - 1):
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        ref = decode_attn_ref(q[None], k[None], v[None], visible_upto([p + 1], cap, device="cuda"))[0]
        y = ops.attn_decode(q, k, v, pos, form="slices256", w=eye).view(nq, 128)
        assert bool(torch.isfinite(y.float()).all())
        e = float((y.float() - ref).abs().max())
        print(f"G={nq // nkv} kv={nkv} pos={p}: max|o - ref| = {e:.3e} (bound {bound:.3e})")
        assert e <= bound, f"G={nq // nkv} kv={nkv} pos={p}: max|o - ref| = {e:.3e} > {bound:.3e}"
        head = ops.attn_decode(q, k, v, pos, form="head")                         # attn_decode_head<false>: the same arguments, the other form
        e = float((head.float() - ref).abs().max())
        assert e <= bound, f"G={nq // nkv} kv={nkv} pos={p}, whole-context form: max|o - ref| = {e:.3e} > {bound:.3e}"


def _bf(t):
    return t.to(torch.bfloat16).float()


def _rms(x, g, eps):
    """HF's RMSNorm on bf16 tensors: bf16(x * rstd) times the gain, rounded again."""
    x32 = x.float()
    return (g * (x32 * torch.rsqrt(x32.pow(2).mean() + eps)).to(torch.bfloat16)).float()


@functools.lru_cache(maxsize=1)
def _one_layer_llm(nq, nkv, hidden, vocab):
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample", layers_l=1)
    c = cfg.llm
    c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.vocab_size = hidden, 1024, nq, nkv, vocab
    c.eos_token_id, cfg.image_token_id, cfg.video_token_id = vocab - 1, vocab - 2, vocab - 3
    cfg.init_std = hidden ** -0.5
    return build_model(cfg, seed=3).llm, c


@pytest.mark.parametrize("nq,nkv,hidden,vocab", [(28, 4, 3584, 1000), (1, 1, 4096, 4100)])
def test_qkv_attention_oproj_chain_inside_a_step(ops, nq, nkv, hidden, vocab):
    llm, c = _one_layer_llm(nq, nkv, hidden, vocab)
    P = {k: v.detach() for k, v in llm.named_parameters()}
    L = "model.layers.0."
    hd, half, cap, eps = 128, 64, 512, c.rms_norm_eps
    cache = llm.new_cache(cap)
    cache.k.copy_(randn_bf16(*cache.k.shape, seed=431, scale=0.5)); cache.v.copy_(randn_bf16(*cache.v.shape, seed=432, scale=0.5))
    st = llm._decode_session(cache, 2)
    tok = torch.tensor([123], dtype=torch.int64, device="cuda")
    x = P["model.embed_tokens.weight"][123]
    xn = _rms(x, P[L + "input_layernorm.weight"], eps)
    proj = {n: _bf(P[L + f"self_attn.{n}_proj.weight"].float() @ xn + P[L + f"self_attn.{n}_proj.bias"].float()) for n in "qkv"}
    inv = 1.0 / torch.pow(torch.tensor(float(c.rope_theta)), torch.arange(half, dtype=torch.float32) * 2 / hd).cuda()
    for p in (0, 255, 256, cap - 1):
        st.pos.fill_(p); st.n_out.zero_(); st.token.copy_(tok)
        llm.decode_step(cache, st)
        torch.cuda.synchronize()
        cs, sn = _bf(torch.cos(p * inv)), _bf(torch.sin(p * inv))

        def rope(t):
            lo, hi = t.view(-1, hd)[:, :half], t.view(-1, hd)[:, half:]
            return torch.cat([_bf(_bf(lo * cs) + _bf(-hi * sn)), _bf(_bf(hi * cs) + _bf(lo * sn))], 1)
        k_ref, v_ref, q_ref = rope(proj["k"]), proj["v"].view(-1, hd), rope(proj["q"])
        for name, got, ref in (("K", cache.k[0, 0, :, p], k_ref), ("V", cache.v[0, 0, :, p], v_ref)):
            e = rel_l2(got, ref)
            print(f"heads {nq}/{nkv} pos {p}: {name} row rel={e:.3e}")
            assert e < BOUND, f"heads {nq}/{nkv} pos {p}: {name} row rel={e:.3e}"
        o = _bf(decode_attn_ref(q_ref.to(torch.bfloat16)[None], cache.k[0], cache.v[0], visible_upto([p + 1], cap, device="cuda"))[0]).reshape(-1)
        h1 = _bf(_bf(P[L + "self_attn.o_proj.weight"].float() @ o) + x.float())
        xn2 = _rms(h1.to(torch.bfloat16), P[L + "post_attention_layernorm.weight"], eps)
        act = _bf(_bf(torch.nn.functional.silu(_bf(P[L + "mlp.gate_proj.weight"].float() @ xn2))) * _bf(P[L + "mlp.up_proj.weight"].float() @ xn2))
        h2 = _bf(_bf(P[L + "mlp.down_proj.weight"].float() @ act) + h1)
        logits = P["lm_head.weight"].float() @ _rms(h2.to(torch.bfloat16), P["model.norm.weight"], eps)
        e = rel_l2(st.logits, logits)
        print(f"heads {nq}/{nkv} pos {p}: logits rel={e:.3e}")
        assert bool(torch.isfinite(st.logits).all()) and e < 2e-2, f"heads {nq}/{nkv} pos {p}: logits rel={e:.3e}"
        assert int(st.token) == int(torch.argmax(st.logits)), f"heads {nq}/{nkv} pos {p}: the fused pick is not the argmax of the logits"
        assert int(st.pos) == p + 1


def test_solo_step_twice_from_one_state(ops):
    """Arguments now arrive by two routes (preloaded SGPRs and the tail's scalar loads); a stale register shows as a run-to-run difference."""
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")                          # head_dim 128, 4 query heads on 2 kv heads
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 0).items()}
    llm = build_model(cfg, weights=w).llm
    S = 10
    ids = torch.randint(0, 900, (S,), generator=torch.Generator().manual_seed(510))
    cache = llm.new_cache(1024)
    _, cache, r, _ = llm._prefill_one(llm.embed_tokens(ids[None].cuda()), None, 2, cache)
    first = ops.argmax(r.last_logits[0])
    st = llm._decode_session(cache, 2)
    got = []
    for _ in range(2):
        st.pos.fill_(S); st.n_out.zero_(); st.token.copy_(first)
        llm.decode_step(cache, st)
        torch.cuda.synchronize()
        assert int(st.pos) == S + 1
        got.append((st.logits.clone(), int(st.token), [t[..., S, :].clone() for t in (cache.k, cache.v)]))
    (lg0, tok0, kv0), (lg1, tok1, kv1) = got
    assert bool(torch.isfinite(lg0).all())
    assert torch.equal(_bits(lg0), _bits(lg1)), "two runs of one step from one state gave different logits"
    assert tok0 == tok1 == int(torch.argmax(lg0.reshape(-1))), "the fused pick is not the argmax of the logits"
    for a, b in zip(kv0, kv1):
        assert bool(torch.isfinite(a.float()).all()) and bool(a.float().abs().sum() > 0), "the step wrote no K/V row at its position"
        assert torch.equal(_bits(a), _bits(b)), "two runs of one step wrote different K/V rows"

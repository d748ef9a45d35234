"""The tail of the batch-1 decode GEMVs ("the tail of a kernel"): the wave reduction without LDS (`wave_sum_xor`: row swaps and
DPP in place of six shuffles) and the K loop split into full batches, requested unpredicated and consumed chunk by chunk behind counted waits,
and a remainder batch whose chunk indices are clamped to the row and whose clamped chunks are replaced by zeros where they are consumed.  Every
output bit is meant to stay.  What can break: a DPP step that reads the wrong partner (the sum of the same 64 values in another association
rounds differently), a batch boundary (a chunk dropped, taken twice, or a clamped chunk that reaches a sum), a register that is consumed before
its load has landed (shows as a run-to-run or grid-to-grid difference).  So:

* the probe export runs both butterflies over 32 waves of inputs whose magnitudes spread over 2^-30 .. 2^30 with mixed signs, with +-0, denormals
  and +-inf planted in single lanes: every lane bit-equal between the two, and bit-equal to a numpy float32 emulation of v += v[lane ^ o],
  o = 32 .. 1; a wave with one NaN lane is NaN in every lane (the payload is not compared: operand order may differ);
* every mode and epilogue of `ops.gemv` (plain, bias + residual, normed, gate/up) and the merge mode through `vila_attn_decode_oproj_bf16`, at
  K = 128 (a remainder batch with fewer chunks than one load instruction), 3584 (exactly one full U = 7 batch; one full + one partial U = 4),
  3592 (one chunk into a second batch), 18944 and 18952 (nine full + one partial U = 4 batch), gate/up also at K = 512, and N = 8 CUs + 3,
  8 CUs + 2, 1000 and 7 — against the fp32 product at the 4e-3 of tests/test_gpu_decode_first_request.py (one bf16 rounding of the output), rows
  bit-equal between the CU-map grid and the small grids.  The weights sit between guard rows of NaN and x between NaN on both sides, as the GEMM
  tests frame theirs: a clamped or masked chunk must never reach an output (the merge mode has no x buffer; its K is whole heads: 128, 3584, 18944);
* the QKV kernel inside a one-layer step (it has no entry point of its own) at head_dim 128, G = 7 and G = 1, positions 0 and 255: the K / V row it
  writes against the fp32 projection through the kernel's roundings at 4e-3, the logits against the fp32 layer at 2e-2 — the bounds of
  tests/test_gpu_decode_first_request.py;
* a tiny-config greedy step twice from one state: the same bits."""
import functools

import numpy as np
import pytest
import torch

from tests.gpu_util import decode_attn_ref, framed_operand, randn_bf16, rel_l2, visible_upto
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu

BOUND = 4e-3          # tests/test_gpu_decode_first_request.py: one bf16 rounding of the output
G_ROWS = 2            # guard rows of NaN on each side of a framed weight matrix


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


# ---- the probe ------------------------------------------------------------------------------------------------------------------------------

def _butterfly(v: np.ndarray) -> np.ndarray:
    """wave_sum on [waves, 64] float32: v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1, every add rounded to float32."""
    lane = np.arange(64)
    v = v.astype(np.float32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[:, lane ^ o]).astype(np.float32)
    return v


def _probe_inputs() -> np.ndarray:
    rng = np.random.default_rng(701)
    mant = rng.uniform(1.0, 2.0, (32, 64))
    expo = rng.integers(-30, 31, (32, 64))
    # waves 0 .. 7 keep a narrow range (the sums of neighbours round; with 60 binades in one wave the largest lane alone decides the sum)
    expo[:8] = rng.integers(-2, 3, (8, 64))
    expo[8:16] = rng.integers(-12, 13, (8, 64))
    sign = rng.choice([-1.0, 1.0], (32, 64))
    v = (sign * mant * np.exp2(expo)).astype(np.float32)
    tiny = np.float32(np.finfo(np.float32).tiny)
    v[16, 5], v[17, 37] = 0.0, -0.0
    v[18, 11], v[18, 50] = tiny / np.float32(4), -tiny / np.float32(64)          # denormals
    v[19, :] = (sign[19] * mant[19]).astype(np.float32) * np.float32(2.0 ** -140)  # a wave of denormals: their sum is one too
    v[20, 63] = np.inf
    v[21, 0] = -np.inf
    v[22, 31], v[22, 32] = 0.0, -0.0
    return v


def test_wave_sum_probe_bits(ops):
    v = _probe_inputs()
    x = torch.from_numpy(v).cuda().contiguous()
    got_xor, got_shfl = (t.cpu().numpy() for t in ops.wave_sum_probe(x.view(-1)))
    got_xor, got_shfl = got_xor.reshape(32, 64), got_shfl.reshape(32, 64)
    ref = _butterfly(v)
    assert not np.isnan(ref).any()
    bad = np.argwhere(got_xor.view(np.uint32) != got_shfl.view(np.uint32))
    assert bad.size == 0, f"wave_sum_xor differs from wave_sum in {len(bad)} lanes, first (wave, lane) {bad[:8].tolist()}"
    bad = np.argwhere(got_xor.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, f"wave_sum_xor differs from the float32 butterfly in {len(bad)} lanes, first (wave, lane) {bad[:8].tolist()}"
    for w in range(32):                       # a butterfly leaves every lane of a wave the same bits only if every step is symmetric: it is
        assert len(set(got_xor[w].view(np.uint32).tolist())) == 1, f"wave {w}: lanes disagree"


def test_wave_sum_probe_nan_lane(ops):
    v = _probe_inputs()[:1].copy()
    v[0, 41] = np.nan
    a, b = ops.wave_sum_probe(torch.from_numpy(v).cuda().view(-1))
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    with pytest.raises(ValueError):
        ops.wave_sum_probe(torch.zeros(65, device="cuda"))


# ---- ops.gemv: every mode and epilogue at the batch boundaries ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _operands(K):
    """x, gain, W (8 CUs + 3 rows), W2, bias, residual and the fp32 products W x, W xn, W2 x, W2 xn — computed once per K.  x is framed by NaN."""
    N = _ns()[0]
    x = framed_operand(randn_bf16(K, seed=701), 0, 2)
    g = randn_bf16(K, seed=702, scale=0.1) + 1
    w = randn_bf16(N, K, seed=703, scale=K ** -0.5)
    w2 = randn_bf16(N, K, seed=704, scale=K ** -0.5)
    b, r = randn_bf16(N, seed=705), randn_bf16(N, seed=706)
    x32 = x.float()
    xn = (g * (x32 * torch.rsqrt(x32.pow(2).mean() + 1e-6)).to(torch.bfloat16)).float()      # HF's rounding order (tests/test_gpu_ops.py)
    return dict(x=x, g=g, w=w, w2=w2, b=b, r=r, wx=w.float() @ x32, wxn=w.float() @ xn, w2x=w2.float() @ x32, w2xn=w2.float() @ xn)


def _framed_rows(w: torch.Tensor, n: int) -> torch.Tensor:
    """The first n rows of w between guard rows of NaN: what lies past the last row (and in front of the first) must never reach an output."""
    v = framed_operand(w[:n], 0, G_ROWS)
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


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


@pytest.mark.parametrize("K", [128, 3584, 3592, 18944, 18952])
def test_plain_gemv_every_epilogue(ops, K):
    d = _operands(K)
    bf = lambda t: t.to(torch.bfloat16).float()
    variants = {
        "plain": (dict(), bf(d["wx"])),
        "fp32 out": (dict(out_f32=True), d["wx"]),
        "norm": (dict(norm_w=d["g"], eps=1e-6), bf(d["wxn"])),
        "bias + residual": (dict(bias=d["b"], residual=d["r"]), bf(bf(d["wx"] + d["b"].float()) + d["r"].float())),
        "norm + residual": (dict(norm_w=d["g"], eps=1e-6, residual=d["r"]), bf(bf(d["wxn"]) + d["r"].float())),
    }
    ws = {n: _framed_rows(d["w"], n) for n in _ns()}
    for name, (kw, ref) in variants.items():
        outs = {}
        for n in _ns():
            kk = {k: (v[:n].contiguous() if k in ("bias", "residual") else v) for k, v in kw.items()}
            outs[n] = ops.gemv(d["x"], ws[n], **kk)
        _check_rows(f"mode 0 {name} K={K}", outs, ref)


@pytest.mark.parametrize("K", [128, 512, 3584, 3592, 18944, 18952])
def test_gate_up_gemv(ops, K):
    """HF: act(gate) * up with every tensor rounded to bf16 — the fp32 products through that chain of roundings."""
    d = _operands(K)
    bf = lambda t: t.to(torch.bfloat16).float()
    ws = {n: (_framed_rows(d["w"], n), _framed_rows(d["w2"], n)) for n in _ns()}
    for name, kw, gk, uk in (("plain", dict(), "wx", "w2x"), ("norm", dict(norm_w=d["g"], eps=1e-6), "wxn", "w2xn")):
        ref = bf(bf(torch.nn.functional.silu(bf(d[gk]))) * bf(d[uk]))
        outs = {n: ops.gemv(d["x"], ws[n][0], w2=ws[n][1], **kw) for n in _ns()}
        _check_rows(f"mode 1 {name} K={K}", outs, ref)


@pytest.mark.parametrize("nq,nkv", [(1, 1), (28, 4), (148, 37)])
def test_merge_gemv_through_attention_and_oproj(ops, nq, nkv):
    """Mode 2 (K = 128, 3584, 18944): x is the merge of the attention partials.  The reference is the fp32 softmax over the visible keys, rounded
    to bf16 as the kernel rounds its merged o, times W in fp32, plus the residual."""
    cap, K = 512, nq * 128
    q, k, v = randn_bf16(nq, 128, seed=711), randn_bf16(nkv, cap, 128, seed=712 + nq), randn_bf16(nkv, cap, 128, seed=713 + nq)
    N = _ns()[0]
    w = randn_bf16(N, K, seed=714, scale=K ** -0.5)
    r = randn_bf16(N, seed=715)
    ws = {n: _framed_rows(w, n) for n in _ns()}
    for p in (300,) if nq == 148 else (10, 300):
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        o = decode_attn_ref(q[None], k[None], v[None], visible_upto([p + 1], cap, device="cuda"))[0]
        ref = ((w.float() @ o.to(torch.bfloat16).float().reshape(-1)).to(torch.bfloat16).float() + r.float()).to(torch.bfloat16).float()
        outs = {n: ops.attn_decode(q, k, v, pos, form="slices256", w=ws[n], residual=r[:n].contiguous()) for n in _ns()}
        _check_rows(f"mode 2 heads={nq} pos={p}", outs, ref)


# ---- QKV inside a step, and a step twice ---------------------------------------------------------------------------------------------------------

def _bf(t):
    return t.to(torch.bfloat16).float()


def _rms(x, g, eps):
    """HF's RMSNorm on bf16 tensors: bf16(x * rstd) times the gain, rounded again."""
    x32 = x.float()
    return (g * (x32 * torch.rsqrt(x32.pow(2).mean() + eps)).to(torch.bfloat16)).float()


@pytest.mark.parametrize("nq,nkv,hidden,vocab", [(28, 4, 3584, 1000), (1, 1, 4096, 4100)])
def test_qkv_inside_a_step(ops, nq, nkv, hidden, vocab):
    """hidden 3584: 2304 row groups on the CU map, one full U = 7 batch per group; hidden 4096: 192 groups on the small grid, two full U = 4
    batches per group (the U = 7 kernels serve K <= 3584)."""
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample", layers_l=1)
    c = cfg.llm
    c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.vocab_size = hidden, 1024, nq, nkv, vocab
    c.eos_token_id, cfg.image_token_id, cfg.video_token_id = vocab - 1, vocab - 2, vocab - 3
    cfg.init_std = hidden ** -0.5
    llm = build_model(cfg, seed=3).llm
    P = {k: v.detach() for k, v in llm.named_parameters()}
    L = "model.layers.0."
    hd, half, cap, eps = 128, 64, 512, c.rms_norm_eps
    cache = llm.new_cache(cap)
    cache.k.copy_(randn_bf16(*cache.k.shape, seed=731, scale=0.5)); cache.v.copy_(randn_bf16(*cache.v.shape, seed=732, scale=0.5))
    st = llm._decode_session(cache, 2)
    tok = torch.tensor([123], dtype=torch.int64, device="cuda")
    x = P["model.embed_tokens.weight"][123]
    xn = _rms(x, P[L + "input_layernorm.weight"], eps)
    proj = {n: _bf(P[L + f"self_attn.{n}_proj.weight"].float() @ xn + P[L + f"self_attn.{n}_proj.bias"].float()) for n in "qkv"}
    inv = 1.0 / torch.pow(torch.tensor(float(c.rope_theta)), torch.arange(half, dtype=torch.float32) * 2 / hd).cuda()
    for p in (0, 255):
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


def test_greedy_step_twice_from_one_state(ops):
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 0).items()}
    llm = build_model(cfg, weights=w).llm
    S = 10
    ids = torch.randint(0, 900, (S,), generator=torch.Generator().manual_seed(710))
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

"""GPU parity tests for the W4A16 decode path (BASELINE configs[4]).

The reference's W4A16 backend (TinyChat / llm-awq) is external and un-vendored, so there is no reference output to pin against:
parity is against the fp32 CPU oracle run on the DEQUANTISED weights — the same numbers the kernels reconstruct in registers.
Model-level cases use weights that are exactly representable in the int4 format (q in 0..15, integer zero, power-of-two scale),
so quantise -> dequantise is the identity and ONE set of weights describes the bf16 prefill, the W4 decode and the oracle.
Tolerances: op level rel-L2 <= 1e-2 (bf16 output rounding), logits rel-L2 <= 3e-2 (the bf16 decode tolerance of test_gpu_model).
"""
import zlib

import pytest
import torch

from oracle import vila_oracle as O
from tests.gpu_util import exact_w4 as _exact_w4, max_abs, rel_l2
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu


def test_quantizer_roundtrip_and_packing():
    from vila_amd.quant import dequantize_w4, quantize_w4, tile_w4
    w = _exact_w4((64, 512), 0)
    q, sz = quantize_w4(w.cuda())
    assert q.shape == (64, 64) and sz.shape == (64, 4) and q.dtype == torch.int32
    assert torch.equal(dequantize_w4(q, sz).cpu(), w)
    qt, szt = tile_w4(q[:37], sz[:37])                   # rows padded to 48 = 3 tiles
    assert qt.numel() == 48 * 64 and szt.numel() == 48 * 4
    # lane 16*g + n of (tile 1, group 2) holds words [8*2*... ] of row 16 + n: k = 256 + 32*g .. + 32
    assert torch.equal(qt.view(3, 4, 4, 16, 4)[1, 2, 3, 5], q[21, 2 * 16 + 3 * 4: 2 * 16 + 3 * 4 + 4])
    assert torch.equal(szt.view(3, 4, 16)[1, 2, 5], sz[21, 2])
    # generic weights: error bounded by half a quantisation step (+ bf16 rounding of the scale)
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(32, 256, generator=g) * 0.05)
    q, sz = quantize_w4(w.cuda())
    d = dequantize_w4(q, sz).cpu()
    step = (w.view(32, 2, 128).amax(-1) - w.view(32, 2, 128).amin(-1)) / 15
    assert ((d - w).view(32, 2, 128).abs().amax(-1) <= 0.52 * step + 1e-6).all()


@pytest.mark.parametrize("N,K", [(3584, 3584), (3584, 18944), (37, 128), (2, 256), (4608, 3584), (512, 1152), (48, 8192)])
@pytest.mark.parametrize("fused", ["plain", "norm_bias_residual"])
def test_gemv_w4_vs_dequantised_fp32(N, K, fused):
    from vila_amd import ops
    from vila_amd.quant import W4Matrix
    g = torch.Generator().manual_seed(N * 7 + K)
    w = torch.randn(N, K, generator=g) * 0.03
    x = torch.randn(K, generator=g).to(torch.bfloat16)
    mat = W4Matrix.pack(w.cuda())
    wd = mat.dequantized().cpu()
    if fused == "plain":
        y = ops.gemv_w4(x.cuda(), mat)
        ref = wd @ x.float()
    else:
        nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
        b = torch.randn(N, generator=g).to(torch.bfloat16)
        r = torch.randn(N, generator=g).to(torch.bfloat16)
        y = ops.gemv_w4(x.cuda(), mat, norm_w=nw.cuda(), eps=1e-6, bias=b.cuda(), residual=r.cuda())
        xn = O.rms_norm(x.float()[None], nw.float(), 1e-6)[0].to(torch.bfloat16).float()
        ref = wd @ xn + b.float() + r.float()
    assert rel_l2(y, ref) < 1e-2, f"rel={rel_l2(y, ref):.3e}"


@pytest.mark.parametrize("N,K", [(18944, 3584), (1152, 512), (5, 128)])
def test_gemv_w4_gate_up(N, K):
    from vila_amd import ops
    from vila_amd.quant import W4Matrix
    g = torch.Generator().manual_seed(N + K)
    wg, wu = torch.randn(N, K, generator=g) * 0.03, torch.randn(N, K, generator=g) * 0.03
    x = torch.randn(K, generator=g).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    mat = W4Matrix.pack(wg.cuda(), wu.cuda())
    y = ops.gemv_w4(x.cuda(), mat, norm_w=nw.cuda(), eps=1e-6)
    assert y.shape == (N,)
    dg, du = mat.dequantized()
    xn = O.rms_norm(x.float()[None], nw.float(), 1e-6)[0].to(torch.bfloat16).float()
    ref = torch.nn.functional.silu(dg.cpu() @ xn) * (du.cpu() @ xn)
    assert rel_l2(y, ref) < 1.5e-2, f"rel={rel_l2(y, ref):.3e}"


def test_gemv_w4_large_offsets_cancel():
    """The kernel computes sum x*(128+q) on the matrix cores and removes the 128- and zero-offsets per group afterwards: an
    activation with a large mean makes that cancellation as hard as it gets."""
    from vila_amd import ops
    from vila_amd.quant import W4Matrix
    g = torch.Generator().manual_seed(11)
    w = torch.randn(256, 1024, generator=g) * 0.02
    x = (3.0 + torch.randn(1024, generator=g)).to(torch.bfloat16)
    mat = W4Matrix.pack(w.cuda())
    y = ops.gemv_w4(x.cuda(), mat)
    ref = mat.dequantized().cpu() @ x.float()
    assert rel_l2(y, ref) < 1e-2, f"rel={rel_l2(y, ref):.3e}"


def test_gemv_w4_rejects_bad_k():
    from vila_amd import ops
    from vila_amd.quant import W4Matrix
    mat = W4Matrix.pack(torch.zeros((4, 256), device="cuda"))
    mat.K = 192
    x = torch.zeros(192, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="multiple of the 128"):
        ops.gemv_w4(x, mat)


def _w4_model(cfg, seed, log2_scale):
    from vila_amd.vlm import build_model
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, seed).items()}
    for k in list(w):
        if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
            w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, log2_scale)
            assert torch.equal(w[k].to(torch.bfloat16).float(), w[k])
    model = build_model(cfg, weights=w)
    q = model.llm.quantize_w4()
    d = q.dequantized_state(model.llm)
    for k, v in d.items():
        assert torch.equal(v, w[k]), f"quantise->dequantise of {k} is not the identity"
    return w, model


def _decode_case(cfg, seed, log2_scale, n_prompt, n_new):
    w, model = _w4_model(cfg, seed, log2_scale)
    px = synthetic.make_pixels(cfg, 1, seed).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, n_prompt, 1, seed)[None]
    e, _, _ = model._embed(ids, {"image": [px[0].cuda()]})
    ids_o, lg_o = O.greedy_generate(e.float().cpu(), w, cfg, n_new, stop_at_eos=False)
    out, lg = model.llm.generate(inputs_embeds=e, max_new_tokens=n_new, return_logits=True, forced_ids=ids_o, use_graph=False)
    err = max_abs(lg, lg_o)
    top2 = lg_o.topk(2, -1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 4 * err
    assert rel_l2(lg, lg_o) < 3e-2, f"W4 decode logits rel={rel_l2(lg, lg_o):.3e}"
    assert torch.equal(out[0].cpu()[decisive], ids_o[decisive])
    # hipGraph replay of the W4 step gives the same ids as the eager launches
    free_e = model.llm.generate(inputs_embeds=e, max_new_tokens=n_new, use_graph=False, eos_token_id=-1)
    free_g = model.llm.generate(inputs_embeds=e, max_new_tokens=n_new, use_graph=True, eos_token_id=-1)
    assert torch.equal(free_e, free_g)
    return model


def test_w4_decode_tiny_vs_oracle():
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152            # K of down_proj must be a multiple of the 128-wide group
    _decode_case(cfg, 3, (-7, -6, -5), 12, 8)


@pytest.mark.parametrize("n_prompt", [16, 560])
def test_w4_decode_8b_widths_vs_oracle(n_prompt):
    """hd = 128: the decode attention runs per-head blocks over 256-key slices and the W4 o_proj kernel merges the slices in its prologue
    (`gemv_w4_kernel<4>`); contexts of 273+ (two slices) and 817+ (four) keys.  The sliced path against the one-block-per-head attention +
    plain W4 o_proj (`vila_decode_force_attn(0)`): same logits up to the merge's rounding."""
    from vila_amd import _lib
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    model = _decode_case(cfg, 5, (-9, -8, -7), n_prompt, 5)
    px = synthetic.make_pixels(cfg, 1, 5).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, n_prompt, 1, 5)[None]
    e, _, _ = model._embed(ids, {"image": [px[0].cuda()]})
    lib = _lib.load()
    try:
        _, lg_sliced = model.llm.generate(inputs_embeds=e, max_new_tokens=5, return_logits=True, use_graph=False, eos_token_id=-1)
        lib.vila_decode_force_attn(0)
        model.llm._drop_decode_session()                       # the eager session holds no captured graph, but start clean
        _, lg_plain = model.llm.generate(inputs_embeds=e, max_new_tokens=5, return_logits=True, use_graph=False, eos_token_id=-1)
    finally:
        lib.vila_decode_force_attn(2)
        model.llm._drop_decode_session()
    assert rel_l2(lg_sliced[1:], lg_plain[1:]) < 1e-2, rel_l2(lg_sliced[1:], lg_plain[1:])
    # (two different kernels really ran: their fp32 merge orders differ, which shows in some bf16 rounding of the 4-slice context; with two
    # slices — one of them 17-22 keys — the hidden states can round identically, as they did once the prefill's q/k/v GEMM changed in round 6)
    assert n_prompt < 560 or not torch.equal(lg_sliced[1:], lg_plain[1:])


def test_w4_refuses_ungrouped_k():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")        # intermediate 1088 is not a multiple of 128
    model = build_model(cfg, seed=0)
    with pytest.raises(AssertionError):
        model.llm.quantize_w4()

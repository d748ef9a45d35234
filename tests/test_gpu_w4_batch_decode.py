"""W4A16 batched decode (vila_gemv_w4_batch_bf16, vila_llm_decode_step_batch_w4, quantize_w4(batch_decode=True)): one pass over the int4
weights serves up to 16 sequences.

Truth is the fp32 dequantise-then-matmul of the SAME quantised weights: at op level `W4Matrix.dequantized`, at model level the CPU oracle on
weights that are exactly representable in the int4 format (so the dequantised model IS the bf16 model).  The batched step sums in another
order than the solo W4 step, so rows are compared with their solo runs under the suite's margin rule (tests/test_gpu_batch_decode.py)."""
import zlib

import pytest
import torch

from oracle import vila_oracle as O
from tests.gpu_util import rel_l2
from tests.test_gpu_batch_decode import _rows_vs_solo
from tests.test_gpu_w4 import _exact_w4
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu

CANARY = -7.25

# ---- op level ---------------------------------------------------------------------------------------------------------------------
_mats = {}


def _mat(N, K, kind):
    from vila_amd.quant import W4Matrix
    key = (N, K, kind)
    if key not in _mats:
        g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        w = (torch.randn(N, K, generator=g) * 0.02).cuda()
        mat = W4Matrix.pack(w, (torch.randn(N, K, generator=g) * 0.02).cuda()) if kind == "gateup" else W4Matrix.pack(w)
        ref = mat.dequantized()
        ref = ref if kind == "gateup" else (ref,)
        bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).cuda()
        _mats.clear()
        _mats[key] = (mat, ref, bias)
    return _mats[key]


def _run(mat, x, bias, residual):
    """ops.gemv_w4_batch into a canary-filled 16-row buffer with a canary tail behind it: returns (y [n, N], whole buffer)."""
    from vila_amd import ops
    n, N = x.shape[0], mat.N
    buf = torch.full((16 * N + 64,), CANARY, device="cuda", dtype=torch.bfloat16)
    out = buf[:16 * N].view(16, N)
    y = ops.gemv_w4_batch(x, mat, bias=bias, residual=residual, out=out)
    assert y.data_ptr() == out.data_ptr()
    return out[:n], buf


def _case(N, K, kind, n, mean=0.0):
    from vila_amd import ops
    mat, ref, bias = _mat(N, K, kind)
    g = torch.Generator().manual_seed(n * 7919 + K)
    x = (mean + torch.randn(n, K, generator=g)).to(torch.bfloat16).cuda()
    xf = x.float()
    if kind == "gateup":
        bias = residual = None
        want = torch.nn.functional.silu(xf @ ref[0].T) * (xf @ ref[1].T)
        bound = 1.5e-2
    else:
        residual = torch.randn(n, N, generator=g).to(torch.bfloat16).cuda()
        want = xf @ ref[0].T + bias.float() + residual.float()
        bound = 1e-2
    y, buf = _run(mat, x, bias, residual)
    assert rel_l2(y, want) < bound, f"n={n} N={N} K={K} {kind}: rel={rel_l2(y, want):.3e}"
    for m in range(n):                                         # each row against the solo W4 GEMV of that row
        solo = ops.gemv_w4(x[m], mat, bias=bias, residual=None if residual is None else residual[m])
        assert rel_l2(y[m], solo) < bound, f"row {m}: vs gemv_w4 rel={rel_l2(y[m], solo):.3e}"
    assert bool((buf[n * N:] == CANARY).all()), "rows >= n or columns >= N were written"
    y2, _ = _run(mat, x, bias, residual)
    assert torch.equal(y, y2), "two calls differ"
    return y


@pytest.mark.parametrize("n", [1, 3, 8, 16])
@pytest.mark.parametrize("N,K,kind", [(3584, 3584, "plain"), (3584, 18944, "plain"), (18944, 3584, "gateup"), (37, 128, "plain"),
                                      (40, 256, "gateup"), (4608, 1152, "plain")])
def test_gemv_w4_batch_vs_dequantised_fp32(N, K, kind, n):
    _case(N, K, kind, n)


@pytest.mark.parametrize("kind", ["plain", "gateup"])
def test_gemv_w4_batch_large_offsets_cancel(kind):
    """sum x * (128 + q) on the matrix cores minus the offsets per group: an activation with a large mean makes that as hard as it gets."""
    _case(256, 1024, kind, 16, mean=3.0)


def test_gemv_w4_batch_rejects_bad_shapes():
    from vila_amd import ops
    mat, _, _ = _mat(37, 128, "plain")
    with pytest.raises(ValueError, match="1..16"):
        ops.gemv_w4_batch(torch.zeros(17, 128, device="cuda", dtype=torch.bfloat16), mat)
    from vila_amd.quant import W4Matrix
    bad = W4Matrix.pack(torch.zeros((4, 256), device="cuda"))
    bad.K = 192
    with pytest.raises(ValueError, match="multiple of the 128"):
        ops.gemv_w4_batch(torch.zeros(2, 192, device="cuda", dtype=torch.bfloat16), bad)


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _model(cfg, seed, log2_scale=None, **qkw):
    """Seeded model; with log2_scale its projections are exactly representable in int4 (the oracle on `w` is then the W4 model)."""
    from vila_amd.vlm import build_model
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, seed).items()}
    if log2_scale is not None:
        for k in list(w):
            if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
                w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, log2_scale)
    model = build_model(cfg, weights=w)
    model.llm.quantize_w4(**qkw)
    return w, model


def _tiny():
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152                 # K of down_proj: a multiple of the 128-wide group
    return cfg


def _8b():
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    return cfg


def _batch(llm, lens, seed, vocab):
    g = torch.Generator().manual_seed(seed)
    L = max(lens)
    ids = torch.randint(0, vocab, (len(lens), L), generator=g)
    mask = torch.zeros(len(lens), L, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, :n] = True
    return llm.embed_tokens(ids.cuda()), mask.cuda()


def _is_w4_session(llm):
    st = getattr(llm, "_bdecode", None)
    return st is not None and st.key[-1] == llm._w4.mats[0]["down"].q.data_ptr()


def _oracle_rows(llm, w, cfg, e, mask, rows, n_new, free):
    """Teacher-forced batched steps (rows in `rows` fed the oracle's ids, the others their free-running ids) against the oracle per row."""
    want = {}
    for b in rows:
        n = int(mask[b].sum())
        want[b] = O.greedy_generate(e[b:b + 1, :n].float().cpu(), w, cfg, n_new, stop_at_eos=False)
    forced = free.clone().cpu()
    for b, (io, _) in want.items():
        forced[b] = io
    got_ids, got_lg = llm._generate_batch(e, mask, n_new, -1, None, use_graph=False, forced_ids=forced, return_logits=True)
    assert _is_w4_session(llm)
    n_dec = 0
    for b, (io, lo) in want.items():
        lg_b = got_lg[:, b].cpu()
        rel = rel_l2(lg_b, lo)
        if rel >= 3e-2:                                       # for the message: the solo W4 step of the same row, teacher-forced alike
            n = int(mask[b].sum())
            _, lg_s = llm.generate(inputs_embeds=e[b:b + 1, :n], max_new_tokens=n_new, return_logits=True, forced_ids=io, use_graph=False)
            rel_s = rel_l2(lg_s.cpu(), lo)
        assert rel < 3e-2, f"row {b} ({int(mask[b].sum())} keys): batched W4 logits vs oracle rel={rel:.3e} (solo W4 step: {rel_s:.3e})"
        # ids: bit-exact at every step whose oracle top-1 / top-2 margin exceeds 4x the observed error (margin_aware_ids' rule); the
        # free-running batch follows the oracle up to the row's first non-decisive step
        err = float((lg_b - lo).abs().max())
        top2 = lo.topk(2, -1).values
        dec = (top2[:, 0] - top2[:, 1]) > 4 * err
        assert torch.equal(lg_b.argmax(-1)[dec], io[dec]), f"row {b}: ids {lg_b.argmax(-1).tolist()} vs oracle {io.tolist()} (decisive {dec.tolist()})"
        nd = (~dec).nonzero().flatten()
        k = int(nd[0]) if nd.numel() else n_new
        assert torch.equal(free[b].cpu()[:k], io[:k]), f"row {b}: free-running {free[b].tolist()} vs oracle {io.tolist()} (first {k} must match)"
        n_dec += int(dec.sum())
    assert n_dec >= 1, "no decisive step in any checked row"


@pytest.mark.parametrize("which", ["tiny", "8b"])
def test_w4_batched_generate_vs_oracle_and_solo_rows(which):
    if which == "tiny":
        # two image + text prompts of test_gpu_w4's tiny case (contexts over 256 and 512 keys: the 8B-width case below; the tiny model's random
        # token rows put even its solo W4 step past the 3e-2 oracle bound)
        cfg = _tiny()
        w, model = _model(cfg, 3, (-7, -6, -5), batch_decode=True)
        px = synthetic.make_pixels(cfg, 1, 3).to(torch.bfloat16)
        ids = synthetic.make_prompt(cfg, 12, 1, 3)[None]
        full = model._embed(ids, {"image": [px[0].cuda()]})[0][0]
        rows = [full, full[:full.shape[0] - 5]]                  # the prompt and a 5-token shorter prefix of it
        L = max(r.shape[0] for r in rows)
        e = torch.zeros(len(rows), L, rows[0].shape[1], device="cuda", dtype=rows[0].dtype)
        mask = torch.zeros(len(rows), L, dtype=torch.bool, device="cuda")
        for b, r in enumerate(rows):
            e[b, :r.shape[0]], mask[b, :r.shape[0]] = r, True
        oracle_rows, n_new = [0, 1], 8
    else:
        cfg = _8b()
        w, model = _model(cfg, 33, (-9, -8, -7), batch_decode=True)
        lens = [600 - 37 * b for b in range(16)]                  # 600 .. 45 keys: one, two and three 256-key slices
        oracle_rows, n_new = [0, 9, 15], 6
        e, mask = _batch(model.llm, lens, 7, 31000)
    llm = model.llm
    both, _, _ = _rows_vs_solo(model, e, mask, n_new)             # batched generate (graph) vs each row's solo W4 generate
    assert _is_w4_session(llm), "the batched W4 step was not taken"
    eager = llm._generate_batch(e, mask, n_new, -1, None, use_graph=False)
    assert torch.equal(eager, both), "graph replay differs from eager launches"
    _oracle_rows(llm, w, cfg, e, mask, oracle_rows, n_new, both)
    # EOS: a row that emits eos stops, the others go on; finished rows are padded
    eos = int(both[0, 2])
    out = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=n_new, eos_token_id=eos, pad_token_id=0)
    row0 = out[0].tolist()
    assert eos in row0 and all(t == 0 for t in row0[row0.index(eos) + 1:])


def test_continuous_batching_on_a_released_w4_model():
    """quantize_w4(prefill=True, release_bf16=True, batch_decode=True): rows join and leave the batched W4 step between steps.  A late row
    and a row that takes over a retired slot decode like their solo W4 runs (test_gpu_batch_decode's continuous-batching case)."""
    cfg = _8b()
    _, model = _model(cfg, 23, prefill=True, release_bf16=True, batch_decode=True)
    llm = model.llm
    g = torch.Generator().manual_seed(23)
    lens = {"A": 40, "B": 300, "C": 17}
    e = {k: llm.embed_tokens(torch.randint(0, 31000, (1, n), generator=g).cuda()) for k, n in lens.items()}
    n_new = 14
    solo = {}
    for k in lens:
        ids, lg = llm.generate(inputs_embeds=e[k], max_new_tokens=n_new, return_logits=True, use_graph=False, eos_token_id=-1)
        top2 = lg.float().topk(2, -1).values
        solo[k] = (ids[0].cpu(), (top2[:, 0] - top2[:, 1]).cpu(), float(lg.float().abs().max()))
    st = llm.batch_open(4, 2048, 64)
    assert _is_w4_session(llm)
    got = {"A": [llm.batch_admit(st, 0, e["A"][0])]}
    llm.batch_run(st, 5)
    got["B"] = [llm.batch_admit(st, 2, e["B"][0])]
    llm.batch_run(st, 8)
    n = st.n_out.tolist()
    assert n[0] == 13 and n[2] == 8
    got["A"] += st.out_ids[0, :13].tolist()
    llm.batch_release(st, [0, 1, 3])
    got["C"] = [llm.batch_admit(st, 0, e["C"][0])]
    llm.batch_run(st, 5)
    n = st.n_out.tolist()
    assert n[0] == 5 and n[2] == 13
    got["B"] += st.out_ids[2, :13].tolist()
    got["C"] += st.out_ids[0, :5].tolist()
    for k, toks in got.items():
        want, margin, top = solo[k]
        bound = 4 * 1.5e-2 * top
        for t, (a, b) in enumerate(zip(toks, want.tolist())):
            if a != b:
                assert float(margin[t]) <= bound, f"row {k} step {t}: {toks} vs solo {want.tolist()} at a decisive step (margin {float(margin[t]):.3f})"
                break
    assert sum(len(v) for v in got.values()) == 14 + 14 + 6


def test_default_quantize_w4_keeps_the_row_by_row_decode():
    """Plain quantize_w4(): generate(batch) runs each row with the solo W4 step (bit-equal ids) and batch_open refuses the model."""
    cfg = _tiny()
    _, model = _model(cfg, 41, (-7, -6, -5))
    llm = model.llm
    assert not llm.can_batch_decode_step()
    e, mask = _batch(llm, [40, 25, 12], 3, 900)
    out = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=6, eos_token_id=-1)
    assert getattr(llm, "_bdecode", None) is None
    for b in range(3):
        solo = llm.generate(inputs_embeds=e[b:b + 1], attention_mask=mask[b:b + 1], max_new_tokens=6, eos_token_id=-1)
        assert torch.equal(out[b], solo[0]), (b, out[b].tolist(), solo[0].tolist())
    with pytest.raises(ValueError):
        llm.batch_open(4, 512, 8)


def test_batched_w4_step_refuses_out_of_range_arguments_before_launching():
    import ctypes as C
    from vila_amd import _lib
    from vila_amd._lib import check
    cfg = _tiny()
    _, model = _model(cfg, 43, (-7, -6, -5), batch_decode=True)
    llm = model.llm
    st = llm.batch_open(4, 512, 8)
    lib = _lib.load()
    w = llm._struct()
    before = (st.pos.clone(), st.n_out.clone(), st.token.clone())

    def step(wc=w, cache=st.cache.c, n=None):
        c = _lib.VilaDecodeBatch.from_buffer_copy(st.c)
        if n is not None:
            c.n = n
        check(lib.vila_llm_decode_step_batch_w4(C.byref(wc), llm._w4.ptr, C.byref(cache), C.byref(c), st.ws.data_ptr(), st.ws.numel(),
                                                None), "vila_llm_decode_step_batch_w4")

    with pytest.raises(ValueError, match="1..16"):
        step(n=17)
    with pytest.raises(ValueError, match=r"cache has 4"):
        step(n=5)
    wbad = _lib.VilaLlmWeights.from_buffer_copy(w)
    wbad.shape.inter = 1088
    with pytest.raises(ValueError, match="multiples of the 128"):
        step(wc=wbad)
    cbad = _lib.VilaKvCache.from_buffer_copy(st.cache.c)
    cbad.max_ctx = 4096
    with pytest.raises(ValueError, match="2048"):
        step(cache=cbad)
    torch.cuda.synchronize()
    for a, b in zip(before, (st.pos, st.n_out, st.token)):
        assert torch.equal(a, b), "a refused step changed the batch state"


def test_serving_w4_batched_model_uses_the_continuous_batcher():
    pytest.importorskip("fastapi")
    from tests.test_gpu_serving import _tokenizer
    from vila_amd import serving
    cfg = _tiny()
    _, model = _model(cfg, 12, (-7, -6, -5), batch_decode=True)
    tok = _tokenizer(cfg)
    app = serving.create_app(model, tok, model_name="NVILA-tiny", batch_window_s=0.01, max_batch=4)
    cb = app.state.batcher
    assert isinstance(cb, serving.ContinuousBatcher)
    try:
        prompts = ["what is this ?", "describe the image", "a red square you are helpful"]
        n = 6
        futs = [cb.submit(p, n, temperature=0.0) for p in prompts]             # concurrent greedy requests
        texts = [f.result(timeout=120) for f in futs]
        assert any(ev[0] == "admit" for ev in cb.events) and _is_w4_session(model.llm)
        eng = serving.HipBatchEngine(model, tok)
        for p, text in zip(prompts, texts):
            e = eng.embed(p, None)
            ids, lg = model.llm.generate(inputs_embeds=e[None], max_new_tokens=n, return_logits=True, use_graph=False, eos_token_id=-1)
            top2 = lg.float().topk(2, -1).values
            margin = (top2[:, 0] - top2[:, 1]).cpu()
            bound = 4 * 1.5e-2 * float(lg.float().abs().max())
            ids = ids[0].tolist()
            k = next((t for t in range(n) if float(margin[t]) <= bound or ids[t] in eng.eos), n)
            want = tok.decode(ids[:k], skip_special_tokens=True).split()
            assert text.split()[:len(want)] == want, (p, text, ids)
    finally:
        cb.close()

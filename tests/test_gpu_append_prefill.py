"""Prefill onto a live KV cache on the GPU: the key-prefix attention (`ops.attn_append`, attn_fwd_kernel's prefix mode, forms A..D through
`vila_attn_force_append`), the C entries `vila_llm_prefill_append` / `_w4` (`llm.prefill_append`), `generate(cache=, past_len=)`,
`generate(prefill_chunk=)` and `serving.ChatSession`.

Bounds are the suite's own: o rel-L2 < O_REL (tests/test_gpu_attention_forms.py) and max|o - ref| <= 2^-7 max|V| (the decode attentions' bound,
tests/test_decode_probe_cpu.py bound_of) against the fp32 softmax over exactly the visible keys; model outputs rel-L2 < 2e-2 against the CPU
oracle (tests/test_gpu_decode_cache_rows.py KV_TOL); ids under the margin-aware rule (tests/gpu_util.py).  The (T, past) cases and the planted keys
are those of tests/test_append_prefill_cpu.py, which proves on the CPU that every planted case discriminates.
VILA_DUMP_PROBE=<file> appends the largest error of every case as a JSON line (the figures in CHANGELOG.md)."""
import contextlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import vila_oracle as O
from tests.gpu_util import decode_attn_ref, margin_aware_ids, max_abs, randn_bf16, rel_l2, visible_upto
from tests.test_append_prefill_cpu import CASES, GROUPS, MAX_CTX, append_probes
from tests.test_decode_probe_cpu import KV, bound_of
from tests.test_gpu_attention_forms import O_REL
from tests.test_gpu_w4 import _exact_w4
from vila_amd import configs, ops, serving, synthetic

pytestmark = pytest.mark.gpu

FORMS = {0: "auto", 1: "A", 2: "B", 3: "C", 4: "D"}
MODEL_TOL = 2e-2


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def _forced(lib, append=0, fwd=0):
    lib.vila_attn_force_append(append)
    lib.vila_attn_force_fwd(fwd)
    try:
        yield
    finally:
        lib.vila_attn_force_append(0)
        lib.vila_attn_force_fwd(0)


def _dump(case, **figures):
    print(f"{case}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))
    path = os.environ.get("VILA_DUMP_PROBE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": case, **figures}) + "\n")


def _append(q, k, v, past, poison_out=True):
    """ops.attn_append into an output pre-filled with 0xFF bytes (bf16 NaN), so that a row the kernel never writes fails every comparison."""
    out = torch.full((q.shape[0], q.shape[1], 128), float("nan"), device=q.device, dtype=torch.bfloat16) if poison_out else None
    return ops.attn_append(q, k, v, past, out=out)


def _q_rows(T, nq, seed):
    """q as the model passes it: rows of a fused [T, (nq + 2 KV) 128] buffer."""
    qkv = randn_bf16(T, (nq + 2 * KV) * 128, seed=seed)
    return qkv[:, :nq * 128].view(T, nq, 128)


# ---- a. the operator against fp32, every form --------------------------------------------------------------------------------------------
_slot = {}


def _random_slot():
    if not _slot:
        _slot["k"], _slot["v"] = randn_bf16(KV, MAX_CTX, 128, seed=21), randn_bf16(KV, MAX_CTX, 128, seed=22)
    return _slot["k"], _slot["v"]


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("T,past", CASES)
def test_operator_against_fp32_softmax_every_form(lib, T, past, G):
    k, v = _random_slot()
    q = _q_rows(T, KV * G, 300 + 7 * T + past + G)
    ref = decode_attn_ref(q, k[None], v[None], visible_upto([past + i + 1 for i in range(T)], MAX_CTX, "cuda"))
    bound = bound_of(v)
    worst_rel = worst_abs = 0.0
    for form, name in FORMS.items():
        with _forced(lib, append=form):
            o = _append(q, k, v, past)
        assert torch.isfinite(o.float()).all(), f"form {name}: rows not written or not finite"
        rel, err = rel_l2(o, ref), max_abs(o, ref)
        worst_rel, worst_abs = max(worst_rel, rel), max(worst_abs, err)
        assert rel < O_REL, f"form {name} T={T} past={past} G={G}: o rel-L2 {rel:.3e}"
        assert err <= bound, f"form {name} T={T} past={past} G={G}: max|o - ref| {err:.3e} > {bound:.3e}"
    _dump(f"append operator T={T} past={past} G={G}", rel_l2=worst_rel, max_abs=worst_abs, bound=bound)


def test_automatic_form_is_the_forwards_policy(lib):
    for T, nq in ((48, 28), (769, 28), (4096, 28), (1, 16)):
        assert lib.vila_attn_append_form(T, nq) == lib.vila_attn_fwd_form(1, T, nq)


# ---- b. planted keys -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("T,past", CASES)
def test_planted_keys_every_form(lib, T, past, G):
    worst = 0.0
    for p in append_probes(G, T, past):
        q, k, v = p.q.cuda(), p.k[0].cuda(), p.v[0].cuda()
        ref = decode_attn_ref(q, k[None], v[None], p.visible(device="cuda"))
        bound = bound_of(p.v)
        for form, name in FORMS.items():
            with _forced(lib, append=form):
                o = _append(q, k, v, past)
            err = float((o.float() - ref).abs().amax((1, 2)).max())
            row = int((o.float() - ref).abs().amax((1, 2)).argmax())
            worst = max(worst, err)
            assert err <= bound, f"{p.name}, form {name}: row {row} (position {past + row}) off by {err:.3e} > {bound:.3e}"
    _dump(f"append planted T={T} past={past} G={G}", max_abs=worst)


# ---- c. poison -----------------------------------------------------------------------------------------------------------------------------
def _poison_rows(t, first):
    """Rows first .. of a [.., max_ctx, 128] cache tensor: NaN, +inf and -inf in turn."""
    if first < t.shape[-2]:
        pat = torch.tensor([float("nan"), float("inf"), float("-inf")], device=t.device).repeat(128)[:128].to(t.dtype)
        t[..., first:, :] = pat


@pytest.mark.parametrize("T,past", [(1, 0), (16, 7), (65, 63), (130, 1), (100, 250), (257, 300)])
def test_rows_beyond_the_sequence_are_never_loaded(lib, T, past):
    k, v = _random_slot()
    q = _q_rows(T, KV * 7, 900 + T)
    kp, vp = k.clone(), v.clone()
    _poison_rows(kp, past + T); _poison_rows(vp, past + T)
    for form, name in FORMS.items():
        with _forced(lib, append=form):
            clean, dirty = _append(q, k, v, past), _append(q, kp, vp, past)
        assert torch.isfinite(dirty.float()).all(), f"form {name}: a poisoned row beyond past + T reached the output"
        assert torch.equal(clean, dirty), f"form {name}: the output depends on rows beyond past + T"


# ---- d. against the existing causal kernel, determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2, 3, 4])
@pytest.mark.parametrize("T,past", [(16, 7), (65, 63), (64, 64), (130, 1), (100, 250), (257, 300)])
def test_rows_are_bit_equal_to_the_one_shot_causal_kernel(lib, T, past, form):
    """The prefix mode keeps attn_fwd_kernel's tile walk (tiles aligned to key 0, the same key groups), so under the same form row i is bit for bit
    the one-shot kernel's row past + i over the same values."""
    L, nq = past + T, KV * 7
    qkv = randn_bf16(L, (nq + 2 * KV) * 128, seed=40 + T)
    q, kk, vv = qkv[:, :nq * 128].view(L, nq, 128), qkv[:, nq * 128:(nq + KV) * 128].view(L, KV, 128), qkv[:, (nq + KV) * 128:].view(L, KV, 128)
    k = torch.zeros((KV, MAX_CTX, 128), device="cuda", dtype=torch.bfloat16)
    v = torch.zeros_like(k)
    k[:, :L], v[:, :L] = kk.transpose(0, 1), vv.transpose(0, 1)
    with _forced(lib, append=form, fwd=form):
        full = ops.attn_fwd(q, kk, vv, causal=True)
        o1, o2 = _append(q[past:], k, v, past), _append(q[past:], k, v, past)
    ref = decode_attn_ref(q, k[None], v[None], visible_upto(range(1, L + 1), MAX_CTX, "cuda"))
    assert rel_l2(full, ref) < O_REL and rel_l2(o1, ref[past:]) < O_REL
    assert torch.equal(o1, o2), "two runs differ"
    assert torch.equal(o1, full[past:]), f"form {FORMS[form]}: rows differ from the one-shot kernel's (max {max_abs(o1, full[past:]):.3e})"


def test_operator_refuses_what_does_not_fit(lib):
    k, v = _random_slot()
    q = _q_rows(8, KV * 7, 1)
    with pytest.raises(ValueError, match="past"):
        ops.attn_append(q, k, v, MAX_CTX - 7)
    with pytest.raises(ValueError, match="past"):
        ops.attn_append(q, k, v, -1)
    o = torch.empty_like(q.contiguous())
    rc = lib.vila_attn_append_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), MAX_CTX - 7, 8, o.data_ptr(), o.stride(0), KV * 7, KV, MAX_CTX,
                                   0.1, ops._stream())
    assert rc != 0 and "exceeds the slot" in lib.vila_last_error().decode()
    rc = lib.vila_attn_append_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), 0, 8, o.data_ptr(), o.stride(0), KV * 7, 3, MAX_CTX, 0.1, ops._stream())
    assert rc != 0 and "multiple of kv heads" in lib.vila_last_error().decode()


# ---- models --------------------------------------------------------------------------------------------------------------------------------
def _weights(cfg, seed, exact_w4):
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, seed).items()}
    if exact_w4:
        for k in list(w):
            if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
                w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, (-9, -8, -7))
    return w


@pytest.fixture(scope="module")
def tiny():
    """configs.tiny (H 512, G 2) on weights that int4 groups of 128 hold exactly (scales 2^-9 .. 2^-7): the bf16 model, the model that prefills from
    its int4 weights, and their common oracle weights."""
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152
    w = _weights(cfg, 3, True)
    vlm = build_model(cfg, weights=w)
    q = build_model(cfg, weights=w).llm
    q.quantize_w4(prefill=True)
    return {"cfg": cfg, "w": w, "vlm": vlm, "bf16": vlm.llm, "w4": q, "vocab": 900, "name": "tiny"}


@pytest.fixture(scope="module")
def wide():
    """configs.reduced_8b: the 8B widths (H 3584, G 7), two layers, bf16."""
    from vila_amd.vlm import build_model
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    w = _weights(cfg, 9, False)
    return {"cfg": cfg, "w": w, "bf16": build_model(cfg, weights=w).llm, "vocab": 31000, "name": "8b"}


@pytest.fixture(scope="module")
def lite():
    """NVILA-Lite-3B widths (H 2048, G 8, tied head), two layers."""
    from vila_amd.vlm import build_model
    cfg = configs.nvila_lite_3b()
    cfg.vision.num_hidden_layers, cfg.llm.num_hidden_layers, cfg.llm.vocab_size = 3, 2, 32000
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    w = _weights(cfg, 11, False)
    return {"cfg": cfg, "w": w, "bf16": build_model(cfg, weights=w).llm, "vocab": 31000, "name": "lite"}


def _prompt(m, S, seed):
    return torch.randint(0, m["vocab"], (S,), generator=torch.Generator().manual_seed(seed))


_oracle = {}


def _oracle_forward(m, ids):
    """The oracle's fp32 forward of the whole sequence, computed once per (model, sequence): logits [S, V], K / V [layers, kv, S, 128], hidden
    states [layers + 1, S, H]."""
    key = (m["name"], tuple(ids.tolist()))
    if key not in _oracle:
        with torch.no_grad():
            logits, past, hs = O.qwen2_forward(O.embed_tokens(ids[None], m["w"]), m["w"], m["cfg"].llm, return_hidden=True)
        _oracle[key] = (logits[0], torch.stack([p[0][0] for p in past]), torch.stack([p[1][0] for p in past]), torch.stack([h[0] for h in hs]))
    return _oracle[key]


def _prefill_then_append(llm, ids, A, cache, slot=0, **want):
    """Tokens 0 .. A - 1 by the one-shot prefill into `slot`, the rest appended.  -> the append's result."""
    e = llm.embed_tokens(ids[None].cuda())[0]
    B = ids.numel() - A
    seq = torch.full((A,), slot, device="cuda", dtype=torch.int32)
    llm.prefill_packed(e[:A], torch.arange(A, device="cuda", dtype=torch.int32), None, A, cache=cache, seq_of_tok=seq)
    last = torch.full((1,), B - 1, device="cuda", dtype=torch.int32)
    return llm.prefill_append(e[A:], cache, A, slot, last_rows=last, **want)


def _against_oracle(case, m, fmt, A, B, max_ctx=512):
    llm = m[fmt]
    assert (llm._w4 is not None and llm._w4_prefill) == (fmt == "w4")
    ids = _prompt(m, A + B, 500 + A + B)
    cache = llm.new_cache(max_ctx)
    r = _prefill_then_append(llm, ids, A, cache, want_layer_hidden=True)
    logits, k_ref, v_ref, hs = _oracle_forward(m, ids)
    fig = {}
    for name, got, ref in (("K", cache.k[:, 0, :, A:A + B], k_ref[:, :, A:]), ("V", cache.v[:, 0, :, A:A + B], v_ref[:, :, A:]),
                           ("hidden", r.layer_hidden, hs[:, A:])):
        for l in range(ref.shape[0]):
            rel = rel_l2(got[l], ref[l])
            fig[name] = max(fig.get(name, 0.0), rel)
            assert rel < MODEL_TOL, f"{case}: {name} of layer {l}, appended rows {A}..{A + B - 1}: rel-L2 {rel:.3e}"
    fig["logits"] = rel_l2(r.last_logits[0], logits[-1])
    _dump(case, **fig)
    assert fig["logits"] < MODEL_TOL, f"{case}: last-row logits rel-L2 {fig['logits']:.3e}"
    # without the taps the last layer is finished for the asked rows alone (prune_last): the same logits to rounding
    cache2 = llm.new_cache(max_ctx)
    r2 = _prefill_then_append(llm, ids, A, cache2)
    assert rel_l2(r2.last_logits[0], logits[-1]) < MODEL_TOL
    assert torch.equal(cache2.k, cache.k) and torch.equal(cache2.v, cache.v)


# ---- f. the model against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "w4"])
@pytest.mark.parametrize("A,B", [(70, 1), (70, 5), (70, 100), (300, 200)])
def test_prefill_then_append_against_the_oracle(tiny, fmt, A, B):
    _against_oracle(f"append model {fmt} tiny A={A} B={B}", tiny, fmt, A, B)


def test_prefill_then_append_against_the_oracle_lite3b_widths(lite):
    assert lite["cfg"].llm.num_attention_heads // lite["cfg"].llm.num_key_value_heads == 8 and lite["cfg"].llm.tie_word_embeddings
    _against_oracle("append model bf16 lite A=70 B=5", lite, "bf16", 70, 5, max_ctx=256)


def test_w4_append_after_release_bf16(tiny):
    from vila_amd.vlm import build_model
    q = build_model(tiny["cfg"], weights=tiny["w"]).llm
    q.quantize_w4(prefill=True, release_bf16=True)
    ids = _prompt(tiny, 75, 575)
    ca, cb = q.new_cache(128), tiny["w4"].new_cache(128)
    ra, rb = _prefill_then_append(q, ids, 70, ca), _prefill_then_append(tiny["w4"], ids, 70, cb)
    assert torch.equal(ra.last_logits, rb.last_logits) and torch.equal(ca.k, cb.k)


# ---- c (model level) and e. poison and footprint on a two-slot cache of the 8B widths ------------------------------------------------------
def test_append_footprint_and_poison_8b_widths(wide):
    llm = wide["bf16"]
    A, B, max_ctx = 37, 21, 128
    ids = _prompt(wide, A + B, 77)
    e = llm.embed_tokens(ids[None].cuda())[0]
    cache = llm.new_cache(max_ctx, n_slots=2)
    other = llm.embed_tokens(_prompt(wide, 50, 78)[None].cuda())[0]
    llm.prefill_packed(other, torch.arange(50, device="cuda", dtype=torch.int32), None, 50, cache=cache)                      # slot 0: another sequence
    llm.prefill_packed(e[:A], torch.arange(A, device="cuda", dtype=torch.int32), None, A, cache=cache,
                       seq_of_tok=torch.ones(A, device="cuda", dtype=torch.int32))
    torch.cuda.synchronize()
    k0, v0 = cache.k.clone(), cache.v.clone()
    last = torch.full((1,), B - 1, device="cuda", dtype=torch.int32)
    clean = llm.prefill_append(e[A:], cache, A, 1, last_rows=last).last_logits.clone()
    torch.cuda.synchronize()
    rows = torch.zeros((2, max_ctx), dtype=torch.bool, device="cuda")
    rows[1, A:A + B] = True
    allowed = rows[None, :, None, :, None]
    for name, now, before in (("K", cache.k, k0), ("V", cache.v, v0)):
        assert torch.equal(now.masked_fill(allowed, 0), before.masked_fill(allowed, 0)), f"{name}: the append wrote outside rows {A}..{A + B - 1} of slot 1"
        changed = (now[:, 1, :, A:A + B] != before[:, 1, :, A:A + B]).any(-1)
        assert bool(changed.all()), f"{name}: (layer, kv head, row) {(~changed).nonzero().tolist()} of the appended rows not written"
    # poison: every row at or beyond A + B of slot 1, in every layer, and the workspace; rows A .. of the slot back to what they were
    k1, v1 = cache.k.clone(), cache.v.clone()
    cache.k.copy_(k0); cache.v.copy_(v0)
    _poison_rows(cache.k[:, 1], A + B); _poison_rows(cache.v[:, 1], A + B)
    llm._ws.fill_(0xFF)
    dirty = llm.prefill_append(e[A:], cache, A, 1, last_rows=last).last_logits
    assert torch.isfinite(dirty).all() and torch.equal(clean, dirty), "poison beyond past + T reached the logits"
    assert torch.equal(cache.k[:, 1, :, :A + B], k1[:, 1, :, :A + B]) and torch.equal(cache.v[:, 1, :, :A + B], v1[:, 1, :, :A + B])


def test_append_entry_refuses_bad_arguments(tiny):
    llm = tiny["bf16"]
    cache = llm.new_cache(64, n_slots=2)
    e = llm.embed_tokens(_prompt(tiny, 10, 1)[None].cuda())[0]
    with pytest.raises(ValueError, match="must fit the KV cache"):
        llm.prefill_append(e, cache, 55)
    with pytest.raises(ValueError, match="slot 2"):
        llm.prefill_append(e, cache, 0, slot=2)
    from vila_amd import _lib
    import ctypes as C
    lib, w = _lib.load(), llm._struct()
    ws = torch.empty((lib.vila_llm_prefill_append_workspace_bytes(C.byref(w.shape), 10),), device="cuda", dtype=torch.uint8)
    call = lambda past, slot: lib.vila_llm_prefill_append(C.byref(w), e.data_ptr(), 10, past, slot, C.byref(cache.c), None, 0, None, None, None,
                                                          ws.data_ptr(), ws.numel(), ops._stream())
    assert call(55, 0) != 0 and "exceeds the KV cache" in lib.vila_last_error().decode()
    assert call(0, 2) != 0 and "outside the cache's 2 slots" in lib.vila_last_error().decode()
    assert call(0, 1) == 0


# ---- g. generate(past_len=) ------------------------------------------------------------------------------------------------------------------
def _two_turns(llm, e1, e2, n1, cache, **first_turn):
    """Turn 1 generated with `first_turn`'s arguments; -> (its ids, the embeddings of turn 2's new tokens = last emitted token + e2, cached)."""
    out1 = llm.generate(inputs_embeds=e1[None], max_new_tokens=n1, eos_token_id=-1, cache=cache, **first_turn)[0]
    assert out1.numel() == n1
    cached = e1.shape[0] + n1 - 1
    new = torch.cat([llm.embed_tokens(out1[-1:][None])[0], e2], 0)
    return out1, new, cached


@pytest.mark.parametrize("fmt", ["bf16", "w4"])
def test_generate_continues_a_cache(tiny, fmt):
    llm = tiny[fmt]
    S1, n1, S2, n2 = 45, 9, 19, 8
    e1 = llm.embed_tokens(_prompt(tiny, S1, 31)[None].cuda())[0]
    e2 = llm.embed_tokens(_prompt(tiny, S2, 32)[None].cuda())[0]
    cache = llm.new_cache(256)
    out1, new, cached = _two_turns(llm, e1, e2, n1, cache)
    assert new.shape[0] == 20
    # the reference: one-shot generate on the whole conversation's embeddings
    whole = torch.cat([e1, llm.embed_tokens(out1[None])[0], e2], 0)
    assert whole.shape[0] == cached + new.shape[0]
    ids_ref, lg_ref = llm.generate(inputs_embeds=whole[None], max_new_tokens=n2, eos_token_id=-1, return_logits=True, use_graph=False)
    ids_got, lg_got = llm.generate(inputs_embeds=new[None], max_new_tokens=n2, eos_token_id=-1, return_logits=True, forced_ids=ids_ref[0],
                                   cache=cache, past_len=cached)
    _dump(f"generate past_len {fmt}", logits_max_abs=max_abs(lg_got, lg_ref), logits_rel_l2=rel_l2(lg_got, lg_ref))
    free = llm.generate(inputs_embeds=new[None], max_new_tokens=n2, eos_token_id=-1, cache=cache, past_len=cached)
    margin_aware_ids(lg_got, lg_ref, ids_ref[0].cpu(), free_ids=free[0])
    assert rel_l2(lg_got, lg_ref) < MODEL_TOL


def test_cached_arithmetic_after_greedy_sampled_and_speculative_first_turns(tiny):
    """After n tokens on a prompt of S the cache holds S + n - 1 valid positions, whatever produced them: the follow-up turn fed from there gives
    the logits of the one-shot prefill of the whole conversation."""
    llm = tiny["bf16"]
    S1, n1, S2 = 45, 12, 19
    ids1 = _prompt(tiny, S1, 41)
    e1 = llm.embed_tokens(ids1[None].cuda())[0]
    e2 = llm.embed_tokens(_prompt(tiny, S2, 42)[None].cuda())[0]
    firsts = {}
    for name, kw in (("greedy", {}), ("sampled", dict(do_sample=True, temperature=0.8, top_k=20, seed=5)),
                     ("lookup", dict(prompt_lookup_num_tokens=4, prompt_ids=ids1.cuda()))):
        cache = llm.new_cache(256)
        out1, new, cached = _two_turns(llm, e1, e2, n1, cache, **kw)
        _poison_rows(cache.k, cached); _poison_rows(cache.v, cached)            # rows beyond the count hold nothing the next turn may read
        whole = torch.cat([e1, llm.embed_tokens(out1[None])[0], e2], 0)
        _, lg_ref = llm.generate(inputs_embeds=whole[None], max_new_tokens=1, eos_token_id=-1, return_logits=True, use_graph=False)
        _, lg_got = llm.generate(inputs_embeds=new[None], max_new_tokens=1, eos_token_id=-1, return_logits=True, cache=cache, past_len=cached)
        assert torch.isfinite(lg_got).all(), f"{name}: rows beyond the cached count were read"
        firsts[name] = (out1, float(rel_l2(lg_got, lg_ref)), lg_got)
        _dump(f"generate past_len after a {name} first turn", first_logits_rel_l2=firsts[name][1])
        assert firsts[name][1] < MODEL_TOL, f"{name}: the follow-up's first logits are {firsts[name][1]:.3e} from the one-shot prefill's"
    # the speculative session emits the plain greedy session's ids, so the second turns start from the same conversation
    assert torch.equal(firsts["lookup"][0], firsts["greedy"][0])
    # ... and its K/V rows, written by the verify step, serve the follow-up as the solo step's do: both sit within MODEL_TOL of the one-shot
    # prefill (above), and of each other
    spec_vs_plain = rel_l2(firsts["lookup"][2], firsts["greedy"][2])
    _dump("generate past_len, speculative against plain first turn", first_logits_rel_l2=spec_vs_plain)
    assert spec_vs_plain < MODEL_TOL, f"speculative vs plain first-token logits {spec_vs_plain:.3e}"


# ---- h. prefill_chunk ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,chunks", [(200, [64, 64, 64, 8]), (65, [64, 1])])
def test_chunked_prefill_follows_the_one_shot_prefill(tiny, S, chunks):
    llm = tiny["bf16"]
    e = llm.embed_tokens(_prompt(tiny, S, 60 + S)[None].cuda())
    n = 8
    ids_ref, lg_ref = llm.generate(inputs_embeds=e, max_new_tokens=n, eos_token_id=-1, return_logits=True, use_graph=False)
    asked, fed = [], []
    ws, pa = llm._workspace, llm.prefill_append
    llm._ws = None
    llm._workspace = lambda nbytes, dev: (asked.append(int(nbytes)), ws(nbytes, dev))[1]
    llm.prefill_append = lambda x, *a, **k: (fed.append((x.shape[0], k.get("last_rows") is not None)), pa(x, *a, **k))[1]
    try:
        ids_got, lg_got = llm.generate(inputs_embeds=e, max_new_tokens=n, eos_token_id=-1, return_logits=True, forced_ids=ids_ref[0], prefill_chunk=64,
                                       cache=llm.new_cache(256))
        free = llm.generate(inputs_embeds=e, max_new_tokens=n, eos_token_id=-1, prefill_chunk=64, cache=llm.new_cache(256))
    finally:
        del llm._workspace, llm.prefill_append
    assert [t for t, _ in fed[:len(chunks) - 1]] == chunks[1:] and [l for _, l in fed[:len(chunks) - 1]] == [False] * (len(chunks) - 2) + [True]
    import ctypes as C
    lib, w = ops._lib.load(), llm._struct()
    # the largest workspace asked for is that of one 64-token chunk: the first chunk's prefill, or an append of 64 where there is one
    ws64 = (lib.vila_llm_prefill_workspace_bytes(C.byref(w.shape), 64), lib.vila_llm_prefill_append_workspace_bytes(C.byref(w.shape), 64))
    assert max(asked) == (ws64[1] if 64 in chunks[1:] else ws64[0]) and max(asked) < lib.vila_llm_prefill_workspace_bytes(C.byref(w.shape), S)
    margin_aware_ids(lg_got, lg_ref, ids_ref[0].cpu(), free_ids=free[0])
    _dump(f"prefill_chunk S={S}", logits_rel_l2=rel_l2(lg_got, lg_ref))
    assert rel_l2(lg_got, lg_ref) < MODEL_TOL


# ---- i. ChatSession ----------------------------------------------------------------------------------------------------------------------------
def _tokenizer(cfg):
    tokenizers = pytest.importorskip("tokenizers")
    transformers = pytest.importorskip("transformers")
    words = ["<unk>", "<|im_start|>", "<|im_end|>", "system", "user", "assistant", "what", "is", "this", "?", "describe", "the", "image", "a",
             "red", "square", "you", "are", "helpful", "and", "colour"]
    words += [f"w{i}" for i in range(min(cfg.image_token_id, cfg.video_token_id, cfg.llm.eos_token_id) - len(words))]
    tk = tokenizers.Tokenizer(tokenizers.models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    tk.pre_tokenizer = tokenizers.pre_tokenizers.WhitespaceSplit()
    return transformers.PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="<unk>", eos_token="<|im_end|>")


def test_chat_session_second_turn_equals_the_one_shot_conversation(tiny):
    cfg, model = tiny["cfg"], tiny["vlm"]
    tok = _tokenizer(cfg)
    img = np.random.default_rng(3).integers(0, 256, size=(56, 56, 3), dtype=np.uint8)
    s = serving.ChatSession(model, tok, max_ctx=256, eos_token_id=-1)
    n1, n2 = 6, 8
    s.ask([img, "what is this ?"], max_new_tokens=n1)
    cached1, ids1 = s.cached, list(s.ids)
    assert ids1.count(cfg.image_token_id) == 1
    reply2 = s.ask("and the colour ?", max_new_tokens=n2)
    conv = s.ids[:-n2]                                                          # what the second reply was generated from, placeholders in
    assert conv[:len(ids1)] == ids1 and s.cached == cached1 + 1 + (len(conv) - len(ids1)) + n2 - 1
    px = serving.preprocess_image(img, cfg.vision.image_size).to(device="cuda", dtype=torch.bfloat16)
    e, _, _ = model._embed(torch.tensor([conv], device="cuda"), {"image": [px]})
    assert e.shape[1] == cached1 + 1 + (len(conv) - len(ids1))
    ids_ref, lg_ref = model.llm.generate(inputs_embeds=e, max_new_tokens=n2, eos_token_id=-1, return_logits=True, use_graph=False)
    # the session's second turn once more, teacher-forced with the one-shot ids, for the logits: the cache still holds the first cached1 positions
    fed = [ids1[-1]] + conv[len(ids1):]
    e_new, _, _ = model._embed(torch.tensor([fed], device="cuda"), {"image": []})
    _, lg_got = model.llm.generate(inputs_embeds=e_new, max_new_tokens=n2, eos_token_id=-1, return_logits=True, forced_ids=ids_ref[0], cache=s.cache,
                                   past_len=cached1)
    decisive = margin_aware_ids(lg_got, lg_ref, ids_ref[0].cpu(), free_ids=torch.tensor(s.ids[-n2:]))
    nd = (~decisive).nonzero().flatten()
    kk = int(nd[0]) if nd.numel() else n2
    assert reply2.split()[:kk] == tok.decode(ids_ref[0].tolist()[:kk], skip_special_tokens=True).split()[:kk]
    with pytest.raises(serving.ChatOverflow):
        s.ask("describe the image", max_new_tokens=250)
    assert s.cached == cached1 + 1 + (len(conv) - len(ids1)) + n2 - 1
    s.reset()
    assert s.cached == 0 and s.ids == []

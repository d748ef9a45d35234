"""What a decode step writes.  A step at position `pos` writes row `pos` of its slot and nothing else, in every layer and kv head, and what it
writes is the K / V of the token it consumed.  Six drivers append K/V during decode, each with its own capacity guard, rotate-half pairing and slot
arithmetic: the solo step (qkv_decode_kernel, gemv_w4 mode 3), the batched step's q/k/v epilogue (bf16 and W4) and the verify step on either
weight format.  For each: the cache is cloned, ONE eager step runs, and
  * footprint: every element outside the expected rows is bit-identical to the clone;
  * contents:  the new rows against the CPU oracle's `past`, teacher-forced on the same tokens, rel-L2 < 2e-2 (the suite's bound for cached K/V
               against the oracle, tests/test_gpu_edge.py) per layer, and for layer 0 — whose input is an exact embedding row — per (kv head, row)
               vector of 128, where one wrong element or rotate-half pair is about 0.1;
  * state:     pos / n_out / token / out_ids move as the driver documents.
Positions: a small one and one past 2000, where more than the first few RoPE pairs have turned.  The W4 models are built from weights that int4
groups of 128 represent exactly (tests/test_gpu_w4_batch_decode.py), so one oracle serves both formats; their group scales are 2^-9 .. 2^-7 (the
8B case of that file, tests/test_gpu_full_size.py).  With 2^-7 .. 2^-5 the tiny model's layer-0 attention is so peaked that a plain PyTorch bf16
forward of it — no kernel of this project involved — already puts a single layer-1 K row 0.6e-2 to 2.1e-2 from the fp32 oracle, astride the
bound; with 2^-9 .. 2^-7 that forward stays within 0.4e-2 .. 1.0e-2 (prompts of 21 and 300 tokens, three seeds each).  The 8B-width model's long position is
checked on layer 0 alone, against a one-token oracle at that position (layer 0's K / V depend on nothing else), which keeps the CPU side quick.
VILA_DUMP_PROBE=<file> appends the largest rel-L2 of every case as a JSON line (the figures in CHANGELOG.md)."""
import json
import os
import zlib

import pytest
import torch

from oracle import vila_oracle as O
from tests.gpu_util import rel_l2
from tests.test_gpu_w4 import _exact_w4
from vila_amd import configs, ops, synthetic

pytestmark = pytest.mark.gpu

KV_TOL = 2e-2


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def _weights(cfg, seed, exact_w4):
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, seed).items()}
    if exact_w4:
        for k in list(w):
            if k.startswith("llm.model.layers.") and k.endswith("_proj.weight"):
                w[k] = _exact_w4(tuple(w[k].shape), zlib.crc32(k.encode()) % 10007, (-9, -8, -7))
    return w


@pytest.fixture(scope="module")
def tiny():
    """configs.tiny (H 512, G 2) on exactly representable weights: the bf16 model, the W4 model and their common oracle weights."""
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    cfg.llm.intermediate_size = 1152                 # K of down_proj: a multiple of the 128-wide group
    cfg.llm.max_position_embeddings = max(getattr(cfg.llm, "max_position_embeddings", 0) or 0, 4096)
    w = _weights(cfg, 3, True)
    q = build_model(cfg, weights=w).llm
    q.quantize_w4(batch_decode=True)
    return {"cfg": cfg, "w": w, "bf16": build_model(cfg, weights=w).llm, "w4": q, "vocab": 900, "name": "tiny"}


@pytest.fixture(scope="module")
def wide():
    """configs.reduced_8b(layers_l=2, vocab=32000): the 8B widths (H 3584, G 7), bf16."""
    from vila_amd.vlm import build_model
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    w = _weights(cfg, 9, False)
    return {"cfg": cfg, "w": w, "bf16": build_model(cfg, weights=w).llm, "vocab": 31000, "name": "8b"}


def _llm(m, fmt):
    llm = m[fmt]
    assert (llm._w4 is not None) == (fmt == "w4")
    return llm


def _prompt(m, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, m["vocab"], (S,), generator=g)


# ---- the oracle's rows -----------------------------------------------------------------------------------------------------------------
_past = {}


def _oracle_rows(m, tokens, first_row, full):
    """K and V [layers, kv, rows, 128] of positions first_row .. len(tokens) - 1 of the sequence `tokens`.  full: the oracle over the whole sequence,
    every layer; otherwise layer 0 only, each token alone at its position (layer 0's K / V are a function of the token and the position)."""
    key = (m["name"], tuple(tokens), first_row, full)
    if key not in _past:
        w, lcfg = m["w"], m["cfg"].llm
        ids = torch.tensor(tokens)
        with torch.no_grad():
            if full:
                _, past = O.qwen2_forward(O.embed_tokens(ids[None], w), w, lcfg)
                k = torch.stack([p[0][0][:, first_row:] for p in past])
                v = torch.stack([p[1][0][:, first_row:] for p in past])
            else:
                rows = torch.arange(first_row, len(tokens))
                _, past = O.qwen2_forward(O.embed_tokens(ids[rows][:, None], w), w, lcfg, position_ids=rows[:, None])
                k, v = past[0][0][:, :, 0].transpose(0, 1)[None], past[0][1][:, :, 0].transpose(0, 1)[None]
        _past.clear()
        _past[key] = (k, v)
    return _past[key]


_worst = {}


def _contents(case, m, cache, slot, rows, tokens, full=True):
    """Rows `rows` (consecutive positions, the last tokens of `tokens`) of `slot` against the oracle."""
    assert rows == list(range(rows[0], rows[0] + len(rows))) and rows[0] + len(rows) <= len(tokens)
    k_ref, v_ref = _oracle_rows(m, tokens[:rows[0] + len(rows)], rows[0], full)
    for name, got_all, ref_all in (("K", cache.k, k_ref), ("V", cache.v, v_ref)):
        for l in range(ref_all.shape[0]):
            got, ref = got_all[l, slot, :, rows[0]:rows[0] + len(rows)].float().cpu(), ref_all[l]
            rel = rel_l2(got, ref)
            _worst[case] = max(_worst.get(case, 0.0), rel)
            assert rel < KV_TOL, f"{case}: {name} of layer {l}, rows {rows[0]}..{rows[-1]} of slot {slot}: rel-L2 {rel:.3e}"
            if l == 0:
                per = (got - ref).norm(dim=-1) / ref.norm(dim=-1)                          # [kv, rows]
                _worst[case] = max(_worst[case], float(per.max()))
                h, r = divmod(int(per.argmax()), per.shape[1])
                assert float(per.max()) < KV_TOL, f"{case}: {name} of layer 0, kv head {h}, row {rows[r]} of slot {slot}: rel-L2 {float(per.max()):.3e}"


def _report(case):
    print(f"{case}: largest K/V rel-L2 against the oracle {_worst.get(case, 0.0):.3e} (bound {KV_TOL:.0e})")
    path = os.environ.get("VILA_DUMP_PROBE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": case, "kv_rel_l2": _worst.get(case, 0.0), "bound": KV_TOL}) + "\n")


# ---- the footprint ---------------------------------------------------------------------------------------------------------------------
def _snapshot(cache):
    torch.cuda.synchronize()
    return cache.k.clone(), cache.v.clone()


def _footprint(case, cache, snap, rows):
    """Outside (slot, row) in `rows` — in any layer and kv head — the cache is bit-identical to the snapshot."""
    torch.cuda.synchronize()
    allowed = torch.zeros((cache.n_slots, cache.max_ctx), dtype=torch.bool, device=cache.k.device)
    for s, r in rows:
        allowed[s, r] = True
    allowed = allowed[None, :, None, :, None]
    for name, now, before in (("K", cache.k, snap[0]), ("V", cache.v, snap[1])):
        a, b = now.masked_fill(allowed, 0), before.masked_fill(allowed, 0)
        if not torch.equal(a, b):
            l, s, h, r, _ = (a != b).nonzero()[0].tolist()
            raise AssertionError(f"{case}: {name} cache changed at layer {l}, slot {s}, kv head {h}, row {r}; the step may write {sorted(rows)}")


def _written(case, cache, snap, slot, rows):
    """Every expected row was written in every layer and kv head (the prefilled caches hold zeros there)."""
    for name, now, before in (("K", cache.k, snap[0]), ("V", cache.v, snap[1])):
        changed = (now[:, slot][:, :, rows] != before[:, slot][:, :, rows]).any(-1)
        assert bool(changed.all()), f"{case}: {name} rows {rows} of slot {slot}: (layer, kv head, row) {(~changed).nonzero().tolist()} not written"


# ---- solo: llm.decode_step -------------------------------------------------------------------------------------------------------------
def _solo(case, m, fmt, S, max_ctx, full=True):
    llm = _llm(m, fmt)
    ids = _prompt(m, S, 100 + S)
    e = llm.embed_tokens(ids[None].cuda())
    cache = llm.new_cache(max_ctx)
    _, cache, r, _ = llm._prefill_one(e, None, 2, cache)
    first = ops.argmax(r.last_logits[0])
    st = llm._decode_session(cache, 2)
    st.pos.fill_(S); st.n_out.zero_(); st.token.copy_(first)
    snap = _snapshot(cache)
    llm.decode_step(cache, st)
    _footprint(case, cache, snap, [(0, S)])
    _written(case, cache, snap, 0, [S])
    assert int(st.pos) == S + 1 and int(st.n_out) == 1, (int(st.pos), int(st.n_out))
    assert int(st.token) == int(st.out_ids[0]) == int(st.logits.argmax())
    _contents(case, m, cache, 0, [S], ids.tolist() + [int(first)], full)
    _report(case)


@pytest.mark.parametrize("S,max_ctx", [(20, 256), (2050, 2304)])
@pytest.mark.parametrize("fmt", ["bf16", "w4"])
def test_solo_step_writes_row_pos_and_nothing_else(tiny, fmt, S, max_ctx):
    """qkv_decode_kernel / gemv_w4 mode 3; 256 positions: the 256-key slices, 2304: the 64-key split."""
    _solo(f"solo {fmt} tiny pos={S}", tiny, fmt, S, max_ctx)


@pytest.mark.parametrize("S,max_ctx,full", [(37, 256, True), (2100, 2304, False)])
def test_solo_step_writes_row_pos_and_nothing_else_8b(wide, S, max_ctx, full):
    _solo(f"solo bf16 8b pos={S}", wide, "bf16", S, max_ctx, full)


def test_solo_driver_refuses_a_cache_without_room(tiny):
    """The solo kernels read pos + 1 keys unguarded; generate() refuses the cache before any launch."""
    llm = tiny["bf16"]
    e = llm.embed_tokens(_prompt(tiny, 20, 1)[None].cuda())
    cache = llm.new_cache(21)
    snap = _snapshot(cache)
    with pytest.raises(ValueError, match="KV cache too small"):
        llm.generate(inputs_embeds=e, max_new_tokens=2, eos_token_id=-1, cache=cache)
    _footprint("refused generate", cache, snap, [])


# ---- batched: llm._batch_step on a batch_open session ------------------------------------------------------------------------------------
def _batched(case, m, fmt, lens, max_ctx, sampled=False, full=(True, True)):
    """Slots 0 and 2 live with different lengths, slot 1 admitted and released, slot 3 never admitted."""
    llm = _llm(m, fmt)
    llm._drop_batch_session()
    st = llm.batch_open(4, max_ctx, 8, sampling=sampled)
    assert st.cache.max_ctx == max_ctx and st.cache.n_slots == 4
    live = {0: _prompt(m, lens[0], 100 + lens[0]), 2: _prompt(m, lens[1], 100 + lens[1])}
    first = {}
    for slot, ids in live.items():
        sp = (0.7, 40, 0.9, 1234) if sampled and slot == 2 else None
        first[slot] = llm.batch_admit(st, slot, llm.embed_tokens(ids[None].cuda())[0], sampling=sp)
    llm.batch_admit(st, 1, llm.embed_tokens(_prompt(m, 29, 7)[None].cuda())[0])
    llm.batch_release(st, [1])
    snap = _snapshot(st.cache)
    with torch.cuda.stream(st.stream):
        llm._batch_step(st)
    st.stream.synchronize()
    rows = [(slot, len(ids)) for slot, ids in live.items()]
    _footprint(case, st.cache, snap, rows + [(1, 0), (3, 0)])                  # an idle row sits at position 0 of its own slot
    pos, n_out = st.pos.tolist(), st.n_out.tolist()
    for i, (slot, ids) in enumerate(live.items()):
        S = len(ids)
        _written(case, st.cache, snap, slot, [S])
        assert pos[slot] == S + 1 and n_out[slot] == 1, (slot, pos, n_out)
        assert int(st.token[slot]) == int(st.out_ids[slot, 0])
        if not (sampled and slot == 2):
            assert int(st.token[slot]) == int(st.logits[slot].argmax())
        _contents(case, m, st.cache, slot, [S], ids.tolist() + [first[slot]], full[i])
    llm._drop_batch_session()
    _report(case)


@pytest.mark.parametrize("fmt,sampled", [("bf16", False), ("w4", False), ("bf16", True)])
def test_batched_step_writes_one_row_per_live_slot(tiny, fmt, sampled):
    """The q/k/v epilogue of decode_batch.hip (bf16) and gemv_w4_batch mode 2 (W4) in a 2304-position session: a row at 2050 and one at 33."""
    _batched(f"batched {fmt}{' sampled' if sampled else ''} tiny pos=2050,33", tiny, fmt, (2050, 33), 2304, sampled)


def test_batched_step_writes_one_row_per_live_slot_8b(wide):
    _batched("batched bf16 8b pos=2100,37", wide, "bf16", (2100, 37), 2304, full=(False, True))


# ---- verify: llm.verify_step -----------------------------------------------------------------------------------------------------------
def _verify_state(llm, cache, n, S, first, cand):
    """A verify session on `cache` in candidate mode, set as generate(prompt_lookup_num_tokens=n - 1, draft_ids=) sets it before its first step."""
    st = llm._verify_session(cache, n, 32, 2)
    st.hist[:1].copy_(first)
    st.cand[:len(cand)].copy_(torch.tensor(cand, dtype=torch.int64))
    st.n_cand.fill_(len(cand))
    st.pos.fill_(S); st.n_out.zero_(); st.n_hist.fill_(1); st.token[:1].copy_(first)
    return st


def _verify(case, m, fmt, S, max_ctx, n=8, full=True):
    llm = _llm(m, fmt)
    ids = _prompt(m, S, 100 + S)
    e = llm.embed_tokens(ids[None].cuda())
    own = llm.generate(inputs_embeds=e, max_new_tokens=n + 1, eos_token_id=-1, use_graph=False)[0].tolist()      # the drafts: the model's own tokens
    cache = llm.new_cache(max_ctx)
    _, cache, r, _ = llm._prefill_one(e, None, n + 1, cache)
    first = ops.argmax(r.last_logits[0])
    assert int(first) == own[0]
    st = _verify_state(llm, cache, n, S, first, own[1:])
    snap = _snapshot(cache)
    llm.verify_step(cache, st)
    _footprint(case, cache, snap, [(0, S + i) for i in range(n)])
    _written(case, cache, snap, 0, list(range(S, S + n)))
    m_acc = int(st.n_accept)
    assert int(st.n_draft) == n - 1 and 0 <= m_acc <= n - 1
    picks = st.logits.argmax(-1).tolist()
    assert picks[:m_acc] == own[1:m_acc + 1], "accepted drafts are the rows' own picks"
    assert int(st.pos) == S + m_acc + 1 and int(st.n_out) == m_acc + 1
    assert st.out_ids[:m_acc + 1].tolist() == picks[:m_acc + 1] and int(st.token[0]) == picks[m_acc]
    print(f"{case}: {m_acc} of {n - 1} drafts accepted")
    assert m_acc >= 1, "no draft accepted: only the committed row would be checked"
    # rows past the accepted run are unspecified; the rows up to it consumed own[0 .. m_acc]
    _contents(case, m, cache, 0, list(range(S, S + m_acc + 1)), ids.tolist() + own[:m_acc + 1], full)
    _report(case)


@pytest.mark.parametrize("S,max_ctx", [(20, 256), (2050, 2304)])
@pytest.mark.parametrize("fmt", ["bf16", "w4"])
def test_verify_step_writes_rows_pos_to_pos_plus_n(tiny, fmt, S, max_ctx):
    _verify(f"verify {fmt} tiny pos={S}", tiny, fmt, S, max_ctx)


@pytest.mark.parametrize("S,max_ctx,full", [(37, 256, True), (2100, 2304, False)])
def test_verify_step_writes_rows_pos_to_pos_plus_n_8b(wide, S, max_ctx, full):
    _verify(f"verify bf16 8b pos={S}", wide, "bf16", S, max_ctx, full=full)


@pytest.mark.parametrize("fmt", ["bf16", "w4"])
def test_verify_step_past_the_capacity_drops_the_rows_that_fall_off(tiny, fmt):
    """pos + n > max_ctx, as generate(max_new_tokens=4, prompt_lookup_num_tokens=7) reaches it on a cache of S + 4 positions: rows 20 .. 23 are
    written, the four that fall off land nowhere — not in the next kv head, not in the next layer — and the committed row is still the oracle's."""
    case = f"verify {fmt} tiny pos=20 of 24"
    llm = _llm(tiny, fmt)
    S, n, max_ctx = 20, 8, 24
    ids = _prompt(tiny, S, 100 + S)
    e = llm.embed_tokens(ids[None].cuda())
    cache = llm.new_cache(max_ctx)
    _, cache, r, _ = llm._prefill_one(e, None, 4, cache)
    first = ops.argmax(r.last_logits[0])
    st = _verify_state(llm, cache, n, S, first, [])
    snap = _snapshot(cache)
    llm.verify_step(cache, st)
    _footprint(case, cache, snap, [(0, S + i) for i in range(max_ctx - S)])
    _written(case, cache, snap, 0, list(range(S, max_ctx)))
    assert int(st.n_draft) == 0 and int(st.n_accept) == 0 and int(st.pos) == S + 1 and int(st.n_out) == 1
    _contents(case, tiny, cache, 0, [S], ids.tolist() + [int(first)])
    _report(case)

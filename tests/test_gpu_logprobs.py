"""Per-token log-probabilities and top alternatives on the device (vila_logprobs_f32, ops.logprobs, generate(logprobs=), batch_open(logprobs=True),
batch_logprobs, score).

Every logprob is compared with the float64 reference (tests/logprob_ref.py) under the per-row bound
    32 * 2^-23 * max(1, max |finite x|, |lse|)
(three roundings at the magnitude of x / lse in x - (M + log L), a summation chain of at most ~40 roundings of relative 2^-24 on L, 1 - 2 ulp in
exp); every id is compared for exact equality with the reference order (value descending, lower index first)."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.gpu_util import framed_operand, framed_out, framed_ws
from tests.logprob_ref import MAX_TOP, bound, check_rows, logprob_ref
from vila_amd import configs

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _width(V):
    from vila_amd import _lib
    return int(_lib.load().vila_logprobs_slice_width(V))


def _raw(lg, token, top_n, rec=None, bias=0, max_rec=2, framed=True, fill=None):
    """The C entry on logits `lg` [n, V] (any row stride): -> (token_lp [n, max_rec], top_lp [n, max_rec, 20], top_id [n, max_rec, 20], checks).
    framed: outputs and workspace lie in patterned frames, `checks` assert them intact.  fill = (f, i): the records' initial values instead."""
    from vila_amd import _lib, ops
    lib = _lib.load()
    n, V = lg.shape
    checks = []
    if framed:
        g = 4                                                          # 4 guard rows of max_rec (* 20) 4-byte elements: 16-byte multiples
        assert max_rec % 2 == 0
        tl, c1 = framed_out(n, max_rec, 0, g, dtype=torch.float32)
        pl, c2 = framed_out(n, max_rec * MAX_TOP, 0, g, dtype=torch.float32)
        pi, c3 = framed_out(n, max_rec * MAX_TOP, 0, g, dtype=torch.int32)
        ws, c4 = framed_ws(int(lib.vila_logprobs_workspace_bytes(n)))
        checks = [c1, c2, c3, c4]
        assert tl.is_contiguous() and pl.is_contiguous() and pi.is_contiguous()
    else:
        tl = torch.empty((n, max_rec), device="cuda", dtype=torch.float32)
        pl = torch.empty((n, max_rec * MAX_TOP), device="cuda", dtype=torch.float32)
        pi = torch.empty((n, max_rec * MAX_TOP), device="cuda", dtype=torch.int32)
        ws = torch.empty((int(lib.vila_logprobs_workspace_bytes(n)),), device="cuda", dtype=torch.uint8)
    if fill is not None:
        tl.fill_(fill[0]); pl.fill_(fill[0]); pi.fill_(fill[1])
    out = _lib.VilaLogprobOut(tl.data_ptr(), pl.data_ptr(), pi.data_ptr(), max_rec)
    rc = lib.vila_logprobs_f32(lg.data_ptr(), lg.stride(0), n, V, token.data_ptr(), top_n, None if rec is None else rec.data_ptr(), bias, C.byref(out),
                               ws.data_ptr(), ops._stream())
    _lib.check(rc, "logprobs")
    torch.cuda.synchronize()
    return tl, pl.view(n, max_rec, MAX_TOP), pi.view(n, max_rec, MAX_TOP), checks


@functools.lru_cache(maxsize=None)
def _random_rows(n, V):
    g = torch.Generator().manual_seed(1000 * n + V)
    x = 4 * torch.randn(n, V, generator=g)
    tok = torch.randint(0, V, (n,), generator=g)
    return x, tok


@functools.lru_cache(maxsize=None)
def _random_ref(n, V):
    return logprob_ref(_random_rows(n, V)[0], MAX_TOP)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the operator against the reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_n", [0, 1, 20])
@pytest.mark.parametrize("n", [1, 3, 16, 40])
@pytest.mark.parametrize("V", [1, 19, 20, 21, 1001, 4099, 152064])
def test_operator_matches_the_float64_reference(V, n, top_n):
    x, tok = _random_rows(n, V)
    lg = framed_operand(x.cuda(), ld_pad=7, guard_rows=1)               # rows V + 7 apart, NaN in the padding columns and the guard rows
    assert lg.stride(0) == V + 7
    tl, pl, pi, checks = _raw(lg, tok.cuda(), top_n, bias=1)            # record 1 of 2
    for c in checks:
        c()
    worst = check_rows(x, tok, tl[:, 1], pl[:, 1], pi[:, 1], top_n, f"V={V} n={n} top_n={top_n}", ref=_random_ref(n, V))
    print(f"V={V} n={n} top_n={top_n}: worst error / bound = {worst:.3f}")
    # the places from top_n on hold id -1 / -inf, whatever the vocabulary
    assert bool((pi[:, 1, top_n:] == -1).all()) and bool((pl[:, 1, top_n:] == -math.inf).all())


def test_a_slice_longer_than_one_chunk():
    """The sizes above keep a slice within the 4096 logits a block holds at a time; a vocabulary beyond 48 * 4096 makes it walk two chunks."""
    V, n = 200003, 2
    assert _width(V) > 4096
    x, tok = _random_rows(n, V)
    x = x.clone()
    w = _width(V)
    x[0, 3 * w + 4096] = 60.0                                           # the maximum in the second chunk of a slice, the runner-up in the first
    x[0, 3 * w + 4095] = 59.0
    x[1, 5 * w + 17] = 60.0                                             # ... and the other way round
    x[1, 5 * w + 4100] = 59.0
    lg = framed_operand(x.cuda(), ld_pad=7, guard_rows=1)
    tl, pl, pi, checks = _raw(lg, tok.cuda(), 20, bias=1)
    for c in checks:
        c()
    check_rows(x, tok, tl[:, 1], pl[:, 1], pi[:, 1], 20, "two chunks, strided rows")
    from vila_amd import ops
    a, b, c = ops.logprobs(x.cuda(), tok.cuda(), 20)                    # tight rows: the 16-byte loads
    check_rows(x, tok, a, b, c, 20, "two chunks, tight rows")
    assert torch.equal(_bits(a), _bits(tl[:, 1])) and torch.equal(_bits(b), _bits(pl[:, 1])) and torch.equal(c.cpu(), pi[:, 1].cpu())


# ----------------------------------------------------------------------------------------------------------------------
# 2. edge rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4099, 152064])
def test_edge_rows(V):
    from vila_amd import ops
    w = _width(V)
    g = torch.Generator().manual_seed(V)
    base = 4 * torch.randn(V, generator=g)
    rows, toks = [], []
    # the maximum at the first and the last element and on both sides of every slice boundary (the runner-up on the other side)
    spots = [(0, V - 1), (V - 1, 0)]
    for k, b in enumerate(range(w, V, w)):
        spots.append((b - 1, b) if k % 2 == 0 else (b, b - 1))
    for hi, lo in spots:
        r = base.clone()
        r[hi], r[lo] = 50.0, 49.5
        rows.append(r); toks.append(hi)
    n_spots = len(rows)
    one = torch.full((V,), -math.inf); one[V // 3] = 2.5                # -inf except one entry: logprob 0 for it
    rows.append(one); toks.append(V // 3)
    holes = base.clone(); holes[torch.rand(V, generator=g) < 0.3] = -math.inf
    holes[0] = -math.inf; holes[V - 1] = -math.inf
    rows.append(holes); toks.append(int(torch.isfinite(holes).nonzero()[5]))
    rows.append(holes); toks.append(0)                                  # the chosen token is a hole: -inf
    rows.append(base + 80); toks.append(7)
    rows.append(base - 80); toks.append(V - 2)
    x, tok = torch.stack(rows), torch.tensor(toks)
    ref = logprob_ref(x, MAX_TOP)
    for name, lg in (("tight", x.cuda()), ("strided", framed_operand(x.cuda(), ld_pad=7, guard_rows=1))):
        tl, pl, pi = ops.logprobs(lg, tok.cuda(), 20)
        check_rows(x, tok, tl, pl, pi, 20, f"V={V} {name}", ref=ref)
        tl, pl, pi = tl.cpu(), pl.cpu(), pi.cpu()
        for r, (hi, lo) in enumerate(spots):
            assert pi[r, 0] == hi and pi[r, 1] == lo, (name, r, hi, lo, pi[r, :2].tolist())
        r = n_spots
        assert float(tl[r]) == 0.0 and pi[r, 0] == V // 3 and float(pl[r, 0]) == 0.0, "one finite entry: logprob 0"
        assert bool((pl[r, 1:] == -math.inf).all()) and pi[r, 1:].tolist() == [i for i in range(20) if i != V // 3][:19], "-inf ties: index order"
        assert float(tl[r + 2]) == -math.inf
        assert bool(torch.isfinite(tl[r + 3:]).all()) and bool(torch.isfinite(pl[r + 3:]).all()), "shifted rows: no overflow, no -inf"
    # a token of -1 and of V: NaN for the chosen logprob, the alternatives unaffected
    bad = tok.clone(); bad[0], bad[1] = -1, V
    tl2, pl2, pi2 = ops.logprobs(x.cuda(), bad.cuda(), 20)
    check_rows(x, bad, tl2, pl2, pi2, 20, f"V={V} bad tokens", ref=ref)
    tl1, pl1, pi1 = ops.logprobs(x.cuda(), tok.cuda(), 20)
    assert torch.equal(_bits(pl2), _bits(pl1)) and torch.equal(pi2, pi1) and torch.equal(_bits(tl2[2:]), _bits(tl1[2:]))


def test_top_20_of_a_vocabulary_of_19():
    from vila_amd import ops
    x, tok = _random_rows(3, 19)
    tl, pl, pi = ops.logprobs(x.cuda(), tok.cuda(), 20)
    check_rows(x, tok, tl, pl, pi, 20, "V=19")
    assert pi[:, 19].tolist() == [-1] * 3 and bool((pl[:, 19] == -math.inf).all()) and bool((pi[:, :19] >= 0).all())


def test_planted_ties_order_towards_the_lower_index():
    from vila_amd import ops
    V = 4099
    x, tok = _random_rows(3, V)
    x = x.clone()
    w = _width(V)
    for r in range(3):
        for i in (5 + r, 6 + r, w - 1, w, 2 * w + 3, V - 1):            # one thread's neighbours, across a slice boundary, the last element
            x[r, i] = 30.0
        x[r, 40], x[r, 41] = 0.0, -0.0                                  # equal as floats: the lower index first
        x[r, 42:60] = -1e30                                             # (keeps the zeros out of reach of the random values below)
    x[2] = torch.where(x[2] < 30.0, torch.full_like(x[2], -1e30), x[2])
    x[2, 41], x[2, 40] = 0.0, -0.0
    tl, pl, pi = ops.logprobs(x.cuda(), tok.cuda(), 20)
    check_rows(x, tok, tl, pl, pi, 20, "ties")
    assert pi[2, :8].tolist() == [7, 8, w - 1, w, 2 * w + 3, V - 1, 40, 41]


@pytest.mark.parametrize("V", [4099, 152064, 200003])
def test_orderings_that_load_the_selection(V):
    """The top 20 of a slice are selected through the 20 threads whose largest logit is largest (thread t of a block owns elements 1024 q + 4 t .. + 3
    of a 4096-logit chunk): rows whose large logits all sit in 20 threads fill its candidate list to the brim, sorted and constant rows make every
    comparison a near tie or a tie."""
    from vila_amd import ops
    w = _width(V)
    g = torch.Generator().manual_seed(7 * V)
    idx = torch.arange(V, dtype=torch.float32)
    base = torch.randn(V, generator=g)
    own = lambda t0: torch.tensor([s0 + 1024 * q + 4 * t + j for s0 in range(0, V, w) for q in range(4) for t in range(t0, t0 + 20) for j in range(4)
                                   if 1024 * q + 4 * t + j < w and s0 + 1024 * q + 4 * t + j < V])
    packed_lo, packed_hi = base.clone(), base.clone()
    packed_lo[own(0)] += 100.0                                          # threads 0 .. 19 of every block hold everything large
    packed_hi[own(236)] += 100.0                                        # ... and threads 236 .. 255
    rows = [idx * 1e-3, -idx * 1e-3, torch.full((V,), 1.25), packed_lo, packed_hi, torch.where(idx % 2 == 0, torch.tensor(3.0), torch.tensor(-3.0))]
    x = torch.stack(rows)
    tok = torch.tensor([V - 1, 0, V // 2, 5, 1000, 2])
    for name, lg in (("tight", x.cuda()), ("strided", framed_operand(x.cuda(), ld_pad=7, guard_rows=1))):
        tl, pl, pi = ops.logprobs(lg, tok.cuda(), 20)
        check_rows(x, tok, tl, pl, pi, 20, f"V={V} {name}")
    assert pi[0].tolist() == list(range(V - 1, V - 21, -1)) and pi[1].tolist() == list(range(20)) and pi[2].tolist() == list(range(20))
    assert pi[5].tolist() == list(range(0, 40, 2))


# ----------------------------------------------------------------------------------------------------------------------
# 3. independence and determinism
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,V", [(16, 152064), (40, 152064), (16, 4099), (40, 4099)])
def test_a_row_does_not_depend_on_its_launch(n, V):
    from vila_amd import ops
    x, tok = _random_rows(n, V)
    lg, tk = x.cuda(), tok.cuda()
    a = ops.logprobs(lg, tk, 20)
    b = ops.logprobs(lg, tk, 20)
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v)), "two launches differ"
    for r in range(n):
        # the same row launched alone, where it lies (V = 4099: 4-byte aligned) and in a buffer of its own (16-byte aligned)
        for alone in (lg[r:r + 1], lg[r:r + 1].clone()):
            s = ops.logprobs(alone, tk[r:r + 1], 20)
            for u, v in zip(a, s):
                assert torch.equal(_bits(u[r:r + 1]), _bits(v)), (n, V, r)


# ----------------------------------------------------------------------------------------------------------------------
# 4. record addressing
# ----------------------------------------------------------------------------------------------------------------------
def test_records_outside_the_buffer_write_nothing():
    V, max_rec = 1001, 4
    rec_h = [0, 1, 5, 3, 0, 2, 4]                                       # with bias -1: -1, 0, 4 (= max_rec), 2, -1, 1, 3
    n = len(rec_h)
    x, tok = _random_rows(n, V)
    rec = torch.tensor(rec_h, dtype=torch.int32, device="cuda")
    FILL_F, FILL_I = 12345.0, -777
    tl, pl, pi, checks = _raw(x.cuda(), tok.cuda(), 20, rec=rec, bias=-1, max_rec=max_rec, fill=(FILL_F, FILL_I))
    for c in checks:
        c()
    ref_t, ref_l, ref_i = _raw(x.cuda(), tok.cuda(), 20, bias=0, max_rec=2, framed=False)[:3]
    tl, pl, pi = tl.cpu(), pl.cpu(), pi.cpu()
    for r in range(n):
        idx = rec_h[r] - 1
        for k in range(max_rec):
            if k == idx:
                assert torch.equal(_bits(tl[r, k]), _bits(ref_t[r, 0])) and torch.equal(_bits(pl[r, k]), _bits(ref_l[r, 0])) and \
                    torch.equal(pi[r, k], ref_i[r, 0].cpu()), (r, k)
            else:
                assert float(tl[r, k]) == FILL_F and bool((pl[r, k] == FILL_F).all()) and bool((pi[r, k] == FILL_I).all()), (r, k, "written")
    # rec NULL: record rec_bias of every row
    tl, pl, pi, _ = _raw(x.cuda(), tok.cuda(), 20, bias=3, max_rec=max_rec, fill=(FILL_F, FILL_I))
    assert bool((tl[:, :3] == FILL_F).all()) and torch.equal(_bits(tl[:, 3]), _bits(ref_t[:, 0])) and bool((pi[:, :3] == FILL_I).all())


def test_bad_arguments_are_refused_before_a_launch():
    from vila_amd import _lib, ops
    lib = _lib.load()
    x, tok = _random_rows(3, 1001)
    lg, tk = x.cuda(), tok.cuda()
    tl = torch.full((3, 1), 5.0, device="cuda"); pl = torch.full((3, 20), 5.0, device="cuda"); pi = torch.full((3, 20), 5, device="cuda", dtype=torch.int32)
    ws = torch.empty((int(lib.vila_logprobs_workspace_bytes(3)),), device="cuda", dtype=torch.uint8)
    full = (tl.data_ptr(), pl.data_ptr(), pi.data_ptr(), 1)

    def call(n=3, top_n=20, ld=1001, o=full):
        out = _lib.VilaLogprobOut(*o)
        return lib.vila_logprobs_f32(lg.data_ptr(), ld, n, 1001, tk.data_ptr(), top_n, None, 0, C.byref(out), ws.data_ptr(), ops._stream())
    assert call() == 0
    tl.fill_(5.0)
    assert call(n=0) != 0 and call(top_n=21) != 0 and call(top_n=-1) != 0 and call(ld=1000) != 0
    assert call(o=(tl.data_ptr(), pl.data_ptr(), None, 1)) != 0 and call(o=(tl.data_ptr(), None, pi.data_ptr(), 1)) != 0
    assert call(top_n=0, o=(tl.data_ptr(), None, None, 1)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.logprobs(lg, tk, 21)
    with pytest.raises(ValueError):
        ops.logprobs(lg, tk[:2], 1)


# ----------------------------------------------------------------------------------------------------------------------
# the sessions, on configs.tiny
# ----------------------------------------------------------------------------------------------------------------------
def _tiny(seed, w4, **quant):
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    if w4:
        cfg.llm.intermediate_size = 1152                               # K of down_proj: a multiple of the 128-wide quantisation group
    model = build_model(cfg, seed=seed)
    if w4:
        model.llm.quantize_w4(**(quant or dict(batch_decode=True)))
    g = torch.Generator().manual_seed(seed)
    L = 20
    ids = torch.randint(0, 900, (3, L), generator=g)
    mask = torch.ones(3, L, dtype=torch.bool); mask[1, 13:] = False; mask[2, 5:] = False
    e = model.llm.embed_tokens(ids.cuda())
    return cfg, model, e, mask.cuda(), [20, 13, 5]


N_NEW = 9
SAMPLING = dict(do_sample=True, temperature=0.9, top_k=30, top_p=0.95)


def _check_lp(lg, ids, lp, b, k, what):
    """Row b of a `Logprobs` against the reference applied to the raw logits lg [n, V] of the steps that chose ids [n]."""
    n = ids.numel()
    assert lp.token_logprobs.dtype == torch.float32 and lp.top_logprobs.dtype == torch.float32 and lp.top_ids.dtype == torch.int64
    return check_rows(lg.float().cpu(), ids.cpu(), lp.token_logprobs[b, :n], lp.top_logprobs[b, :n], lp.top_ids[b, :n], k, what)


# 5. solo
@pytest.mark.parametrize("w4,case", [(False, "greedy"), (False, "sampled"), (True, "greedy"), (True, "sampled"), (False, "penalised-sampled")],
                         ids=["bf16-greedy", "bf16-sampled", "w4-greedy", "w4-sampled", "bf16-penalised-sampled"])
def test_solo_generate_returns_the_raw_logprobs_of_its_tokens(w4, case):
    cfg, model, e, mask, lens = _tiny(51, w4)
    llm, V = model.llm, cfg.llm.vocab_size
    kw = dict(inputs_embeds=e[:1], max_new_tokens=N_NEW, eos_token_id=-1)
    if case != "greedy":
        kw.update(SAMPLING, seed=321)
    if case == "penalised-sampled":
        kw.update(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)
    plain = llm.generate(**kw)
    assert isinstance(plain, torch.Tensor) and llm._decode.lp is None and "logprobs" not in llm._decode.key
    ids, lp = llm.generate(**kw, logprobs=20)
    sess = llm._decode
    assert sess.lp is not None and "logprobs" in sess.key and sess.graph is not None
    assert torch.equal(ids, plain), "logprobs changed the ids"
    assert lp.token_logprobs.shape == (1, N_NEW) and lp.top_logprobs.shape == (1, N_NEW, 20) and lp.top_ids.shape == (1, N_NEW, 20)
    # a smaller k is a slice of the same records, from the same graph; eager steps give the same bits
    ids5, lp5 = llm.generate(**kw, logprobs=5)
    assert llm._decode is sess and torch.equal(ids5, plain) and lp5.top_ids.shape == (1, N_NEW, 5)
    assert torch.equal(_bits(lp5.token_logprobs), _bits(lp.token_logprobs)) and torch.equal(lp5.top_ids, lp.top_ids[:, :, :5])
    ids_e, lp_e = llm.generate(**kw, logprobs=20, use_graph=False)
    assert torch.equal(ids_e, plain) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(lp_e[:2], lp[:2])) and torch.equal(lp_e.top_ids, lp.top_ids)
    ids0, lp0 = llm.generate(**kw, logprobs=0)
    assert lp0.top_logprobs.shape == (1, N_NEW, 0) and torch.equal(_bits(lp0.token_logprobs), _bits(lp.token_logprobs))
    # a run that ends at an EOS early: the records are cut where the ids are
    eos = int(plain[0, 3])
    m = plain[0].tolist().index(eos) + 1
    ids_c, lp_c = llm.generate(**dict(kw, eos_token_id=eos), logprobs=20)
    assert ids_c.shape == (1, m) and torch.equal(ids_c[0], plain[0, :m])
    assert lp_c.token_logprobs.shape == (1, m) and lp_c.top_ids.shape == (1, m, 20)
    assert torch.equal(_bits(lp_c.token_logprobs), _bits(lp.token_logprobs[:, :m])) and torch.equal(lp_c.top_ids, lp.top_ids[:, :m])
    # the raw logits of the same request, step by step (the ids fed are the ones it chose; an unflagged session takes the flagged one's place)
    ids_r, lg = llm.generate(**kw, return_logits=True, forced_ids=plain[0])
    assert llm._decode.lp is None and torch.equal(ids_r, plain) and lg.shape == (N_NEW, V)
    _check_lp(lg, plain[0], lp, 0, 20, f"solo {case}")


# 6. batched
@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4"])
def test_a_padded_batch_returns_logprobs_with_padding_behind_eos(w4):
    cfg, model, e, mask, lens = _tiny(53, w4)
    llm, V = model.llm, cfg.llm.vocab_size
    kw = dict(inputs_embeds=e, attention_mask=mask, max_new_tokens=N_NEW, eos_token_id=-1)
    plain = llm.generate(**kw)
    assert llm._bdecode.lp is None and "logprobs" not in llm._bdecode.key
    ids, lp = llm.generate(**kw, logprobs=5)
    assert llm._bdecode.lp is not None and "logprobs" in llm._bdecode.key and llm._bdecode.graph is not None
    assert torch.equal(ids, plain) and lp.top_ids.shape == (3, N_NEW, 5)
    _, lg = llm._generate_batch(e, mask, N_NEW, -1, None, use_graph=False, forced_ids=plain, return_logits=True)      # [n_new, B, V], raw
    for b in range(3):
        _check_lp(lg[:, b], plain[b], lp, b, 5, f"batch row {b}")
    # row 0 ends early at an EOS: its pad positions hold 0.0 / -inf / -1, everything in front keeps its bits
    eos = int(plain[0, 2])
    cut = [r.index(eos) + 1 if eos in r else N_NEW for r in plain.tolist()]
    ids_c, lp_c = llm.generate(**dict(kw, eos_token_id=eos), logprobs=5)
    n_cols = max(cut)
    assert ids_c.shape == (3, n_cols) and min(cut) < n_cols, cut
    for b in range(3):
        m = cut[b]
        assert torch.equal(ids_c[b, :m], plain[b, :m])
        assert torch.equal(_bits(lp_c.token_logprobs[b, :m]), _bits(lp.token_logprobs[b, :m])) and torch.equal(lp_c.top_ids[b, :m], lp.top_ids[b, :m])
        assert torch.equal(_bits(lp_c.top_logprobs[b, :m]), _bits(lp.top_logprobs[b, :m]))
        assert bool((lp_c.token_logprobs[b, m:] == 0.0).all()) and bool((lp_c.top_logprobs[b, m:] == -math.inf).all()) and bool((lp_c.top_ids[b, m:] == -1).all())


def test_num_return_sequences_sums_to_the_reference():
    cfg, model, e, mask, lens = _tiny(55, False)
    llm, V, n_new = model.llm, cfg.llm.vocab_size, 6
    ep = llm.embed_tokens(torch.randint(0, 900, (1, 300), generator=torch.Generator().manual_seed(3)).cuda())
    kw = dict(inputs_embeds=ep, max_new_tokens=n_new, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=30, top_p=0.95, seed=21, batch_sample=True,
              num_return_sequences=3)
    plain = llm.generate(**kw)
    ids, lp = llm.generate(**kw, logprobs=5)
    st = llm._bdecode
    assert st.shared_prefix and st.S == 256 and st.lp is not None and st.sampling
    assert torch.equal(ids, plain) and lp.token_logprobs.shape == (3, n_new)
    ids_r, lg = llm.generate(**kw, return_logits=True)                  # eager steps of the same request: [n_new, 3, V]
    assert torch.equal(ids_r, plain)
    for b in range(3):
        _check_lp(lg[:, b], plain[b], lp, b, 5, f"sample {b}")
        ref_lp, lse, _, _ = logprob_ref(lg[:, b].cpu(), 0)
        want = float(ref_lp[torch.arange(n_new), plain[b].cpu()].sum())
        assert abs(float(lp.token_logprobs[b].double().sum()) - want) <= float(bound(lg[:, b].cpu(), lse).sum()), (b, want)


def test_an_open_batch_keeps_every_rows_own_records():
    cfg, model, e, mask, lens = _tiny(57, False)
    llm, V = model.llm, cfg.llm.vocab_size
    prompts = {0: e[0, :20], 1: e[1, :13], "again": e[2, :5]}

    def first_logits(x, slot):
        """The prefill's last row exactly as batch_admit computes it (into a cache of its own)."""
        P = x.shape[0]
        c = llm.new_cache(256, n_slots=3)
        r = llm.prefill_packed(x.to(llm.dtype), torch.arange(P, device="cuda", dtype=torch.int32), torch.tensor([0, P], device="cuda", dtype=torch.int32), P,
                               cache=c, seq_of_tok=torch.full((P,), slot, device="cuda", dtype=torch.int32),
                               last_rows=torch.full((1,), P - 1, device="cuda", dtype=torch.int32))
        return r.last_logits[0].clone()

    def run(graph):
        """Row 0 joins; 3 steps; row 1 joins; 5 steps; row 1 leaves and another request takes its slot; 2 steps.  -> per request (ids, records,
        the raw logits of its steps), the logits only from eager steps."""
        st = llm.batch_open(3, 256, 16, logprobs=True)
        llm.batch_release(st, [0, 1, 2])
        steps_lg = {0: [], 1: [], "again": []}

        def go(k, live):
            if graph:
                llm.batch_run(st, k)
                return
            torch.cuda.current_stream().synchronize()
            with torch.cuda.stream(st.stream):
                for _ in range(k):
                    llm._batch_step(st)
                    for name, row in live.items():
                        steps_lg[name].append(st.logits[row].clone())
            st.stream.synchronize()
        f0 = llm.batch_admit(st, 0, prompts[0])
        go(3, {0: 0})
        f1 = llm.batch_admit(st, 1, prompts[1])
        go(5, {0: 0, 1: 1})
        first_run = ([f1] + st.out_ids[1, :5].tolist(), llm.batch_logprobs(st, 1))
        llm.batch_release(st, [1])
        f2 = llm.batch_admit(st, 1, prompts["again"])
        go(2, {0: 0, "again": 1})
        out = {0: ([f0] + st.out_ids[0, :10].tolist(), llm.batch_logprobs(st, 0)), 1: first_run,
               "again": ([f2] + st.out_ids[1, :2].tolist(), llm.batch_logprobs(st, 1))}
        return st, out, steps_lg

    st, eager, lgs = run(False)
    assert st.lp is not None and "logprobs" in st.key
    for name, slot in ((0, 0), (1, 1), ("again", 1)):
        ids, lp = eager[name]
        lg = torch.stack([first_logits(prompts[name], slot)] + lgs[name])
        assert lp.token_logprobs.shape == (len(ids),) and lp.top_ids.shape == (len(ids), 20), (name, lp.token_logprobs.shape)
        check_rows(lg.cpu(), torch.tensor(ids), lp.token_logprobs, lp.top_logprobs, lp.top_ids, 20, f"request {name}")
    assert eager["again"][1].token_logprobs.numel() == 3, "a re-used slot shows the former request's records"
    # the captured graph records the same bits
    st2, graph, _ = run(True)
    assert st2 is st and st.graph is not None
    for name in eager:
        assert graph[name][0] == eager[name][0]
        for a, b in zip(graph[name][1], eager[name][1]):
            assert torch.equal(_bits(a.float()), _bits(b.float())), name
    # a session without the flag has no records and the key it always had
    plain = llm.batch_open(3, 256, 16)
    assert plain is not st and plain.lp is None and "logprobs" not in plain.key
    with pytest.raises(ValueError, match="logprobs=True"):
        llm.batch_logprobs(plain, 0)


# 7. one graph
def test_one_captured_graph_serves_every_logprob_request():
    cfg, model, e, mask, lens = _tiny(59, False)
    llm = model.llm
    kw = dict(max_new_tokens=N_NEW, eos_token_id=-1)
    a, la = llm.generate(inputs_embeds=e[:1], logprobs=3, repetition_penalty=1.3, **kw)
    sess, graph = llm._decode, llm._decode.graph
    assert sess.lp is not None and sess.pen is not None and graph is not None
    b, lb = llm.generate(inputs_embeds=e[:1], logprobs=20, presence_penalty=0.7, frequency_penalty=-1e4, **kw)
    assert llm._decode is sess and llm._decode.graph is graph, "another top_logprobs / other penalties re-captured the graph"
    assert la.top_ids.shape == (1, N_NEW, 3) and lb.top_ids.shape == (1, N_NEW, 20) and not torch.equal(a, b)
    # the batched sampling session: other sampling parameters and another k
    bk = dict(inputs_embeds=e, attention_mask=mask, do_sample=True, batch_sample=True, seed=5, **kw)
    c, lc = llm.generate(temperature=0.9, top_k=30, top_p=0.95, logprobs=2, **bk)
    bsess, bgraph = llm._bdecode, llm._bdecode.graph
    assert bsess.lp is not None and bsess.sampling and bgraph is not None
    d, ld = llm.generate(temperature=0.5, top_k=10, top_p=1.0, logprobs=7, **bk)
    assert llm._bdecode is bsess and llm._bdecode.graph is bgraph
    assert lc.top_ids.shape == (3, N_NEW, 2) and ld.top_ids.shape == (3, N_NEW, 7)
    # sessions opened without the flag beside them have the keys they always had
    llm.generate(inputs_embeds=e[:1], **kw)
    assert llm._decode is not sess and llm._decode.lp is None
    assert llm._decode.key == (llm._decode.cache.k.data_ptr(), N_NEW, *llm._weights_key()[:2], None)
    llm.generate(inputs_embeds=e, attention_mask=mask, **kw)
    assert llm._bdecode is not bsess and llm._bdecode.lp is None
    assert llm._bdecode.key == (3, 256, N_NEW, False, *llm._weights_key())


# 8. score
@pytest.mark.parametrize("w4", [False, True], ids=["bf16", "w4-prefill"])
def test_score_gives_the_log_likelihood_of_a_given_continuation(w4):
    cfg, model, e, mask, lens = _tiny(61, w4, prefill=True)
    llm, V, S, T = model.llm, cfg.llm.vocab_size, 60, 40
    ids = torch.randint(0, 900, (S,), generator=torch.Generator().manual_seed(8))
    x = llm.embed_tokens(ids.cuda())
    lp = llm.score(x, ids[-T:], top_n=5)
    assert lp.token_logprobs.shape == (T,) and lp.top_logprobs.shape == (T, 5) and lp.top_ids.shape == (T, 5) and lp.top_ids.dtype == torch.int64
    r = llm.prefill_packed(x.to(llm.dtype), torch.arange(S, device="cuda", dtype=torch.int32), None, S, want_all_logits=True)
    lg = r.all_logits[S - T - 1:S - 1]                                  # row p predicts the token at p + 1
    check_rows(lg.cpu(), ids[-T:], lp.token_logprobs, lp.top_logprobs, lp.top_ids, 5, "score")
    assert lp.token_logprobs.sum() < 0
    lp0 = llm.score(x, ids[-T:].cuda())
    assert lp0.top_ids.shape == (T, 0) and torch.equal(_bits(lp0.token_logprobs), _bits(lp.token_logprobs))
    for bad, why in ((ids[:0], "target ids"), (torch.zeros(513, dtype=torch.int64), "target ids"), (ids, "LAST positions")):
        with pytest.raises(ValueError, match=why):
            llm.score(x, bad)
    with pytest.raises(ValueError, match="top_n"):
        llm.score(x, ids[-T:], top_n=21)


def test_the_solo_session_serves_a_chunked_prefill_and_a_continued_cache():
    cfg, model, e, mask, lens = _tiny(63, False)
    llm, V = model.llm, cfg.llm.vocab_size
    kw = dict(inputs_embeds=e[:1], max_new_tokens=N_NEW, eos_token_id=-1, prefill_chunk=8)
    plain = llm.generate(**kw)
    ids, lp = llm.generate(**kw, logprobs=4)
    assert torch.equal(ids, plain) and llm._decode.lp is not None and lp.top_ids.shape == (1, N_NEW, 4)
    # a second turn onto the cache the first one left: 20 prompt positions and N_NEW - 1 fed tokens are cached
    cache, past = llm._decode.cache, 20 + N_NEW - 1
    turn = dict(inputs_embeds=llm.embed_tokens(plain[:, -1:]), max_new_tokens=5, eos_token_id=-1, cache=cache, past_len=past)
    ids2, lp2 = llm.generate(**turn, logprobs=4)
    _, lg = llm.generate(**dict(kw), return_logits=True, forced_ids=plain[0])
    _check_lp(lg, plain[0], lp, 0, 4, "chunked prefill")
    # (the return_logits run re-filled the same cache with the same prompt and ids: the second turn again, for its raw logits)
    ids2_r, lg2 = llm.generate(**turn, return_logits=True, forced_ids=ids2[0])
    assert torch.equal(ids2_r, ids2) and lp2.token_logprobs.shape == (1, 5)
    _check_lp(lg2, ids2[0], lp2, 0, 4, "continued cache")

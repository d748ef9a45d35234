"""Every element of the batched decode's skinny GEMM (bgemm_dma_kernel, vila_amd/csrc/decode_batch.hip) against a derived bound, in framed buffers.

The kernel serves every bf16 projection of the batched, verify and shared-prefix steps, which judge it by the rel-L2 of a logits row through 2+
layers (tol_rel = 1.5e-2).  A fault confined to one tile edge, one lane group, one wave's last k-block or one parity buffer fits inside that
(tests/test_batch_gemm_bound_cpu.py shows which ones).  Here the kernel is launched alone through vila_gemm_batch_bf16 / vila_qkv_batch_bf16, which
fill a BGemmArgs and call the step's own launch_bgemm.  Each case
  - reads x through a view with ldx = K + 8, NaN padding and NaN guard rows (rows beyond the batch are copies of row n - 1, decode_batch.hip:159);
    W (and W2) with the row stride K the kernel assumes and NaN guard rows before row 0 and behind row N - 1 (the clamp of decode_batch.hip:174
    must keep the reads inside); bias and residual (ldr = N + 8) framed the same way;
  - writes views of 16 rows with ldy / ldf / ldq = N + 8 inside buffers that hold a bit pattern, only n rows in use: after the call every element
    outside the n x N view is the pattern bit for bit; the KV caches are [16 slots][kv][8][head_dim] of the pattern between guard slots, and
    the only elements that may differ afterwards are (slot m, every kv head, row pos[m]) of rows with pos[m] < 8;
  - checks every element against an fp64 reference of the same bf16 inputs under the bounds of tests/gpu_util.py, which follow the roundings of
    bgemm_epilogue: plain decode_batch.hip:100-104 (fp32 as summed: A; bf16: 2^-8 |ref| + A; with residual, line 103, 2^-8 |core + bias| +
    2^-8 |ref| + A), gate/up decode_batch.hip:57-58 with common.h:61 silu_f (bgemm_gateup_bound), q|k|v decode_batch.hip:72-77
    (bgemm_qkv_bound).  A = (1 + 2^-8) (K + 10) 2^-24 |x| . |W| (+ |bias| + |residual|): K products, the adds of the 8 wave partials
    (decode_batch.hip:232-235), bias and residual;
  - runs twice, bit-equal; and row m of the n-row call is bit-equal to that row computed alone (n = 1) and to row m of a 16-row call: an MFMA
    output row depends on its own A row only (decode_batch.hip:209-214), and the order of the k-blocks (wave w: w, w + 8, ...; partials 0..7)
    depends on K alone.

Shapes, the smallest at which each mechanism engages: n in {1, 4, 5, 8, 9, 16} (the 8 -> 16 row activation slice of launch_bgemm's x8, the quads
of the C layout, the full tile); K in {64 (one k-block, seven waves without one), 448 (one idle wave), 512, 576 and 1088 (9 and 17 k-blocks,
uneven shares), 3136 (49: wave 0 has 7, more than any ring depth NS <= 5, every ring wraps)}; N in {4, 20 (clamped last tile), 16, 4100 (257 items:
block 0 walks two, the second clamped), 8200 (513 items: three on block 0, both parities reused)}; K rotates over (n, N), K <= 1088 at
N >= 4100 but for one (16, 8200, 3136).  q|k|v heads (2, 1, 32) (one item per head), (3, 1, 64), (28, 4, 128) (144 items), (60, 4, 128) (272
items: blocks walk).

The W4A16 sibling (vila_gemv_w4_batch_bf16, modes 0 and 1) goes through the same framed x, bias, residual and 16-row output: every element against
the dequantised fp64 product under w4_generic_bound (tests/gpu_util.py; tests/test_gpu_w4_elements.py has the kernel's own shapes and the exact
regime), and every row and every column by rel-L2 at its own test's bounds (1e-2 plain, 1.5e-2 gate/up); its entry point takes no ldr / ldy, so
those two are framed by guard rows only."""
import itertools

import pytest
import torch

from tests.gpu_util import (assert_elementwise, assert_qkv_outputs, bgemm_gateup_bound, bgemm_plain_bound, bgemm_qkv_bound, framed_cache, framed_operand,
                            framed_out_rows, rope_table, w4_generic_acc, w4_generic_bound, w4_unpack)

pytestmark = pytest.mark.gpu

G = 4                                                    # guard rows on each side of every framed operand and output
NS_ROWS = (1, 4, 5, 8, 9, 16)
KS = (64, 448, 512, 576, 1088, 3136)
NS_COLS = (4, 16, 20, 4100, 8200)
EPILOGUES = ("none", "bias", "residual", "bias+residual", "inplace", "f32", "both")
INDEPENDENCE_EPILOGUES = ("bias+residual", "both")       # the ones whose rows are also computed alone: one bf16 and the fp32 output
HEADS = ((2, 1, 32), (3, 1, 64), (28, 4, 128), (60, 4, 128))
QKV_KS = (64, 576, 1088)
MAX_CTX = 8
# cache rows; 8 = max_ctx and 13 = max_ctx + 5 write q and no K/V.  Were such a row stored, it would land at row 0 / row 5 of the next kv head or, from the
# last head, of the next slot: the next slot's own position is neither (5, 7, 2, 6, 4 behind rows 1, 3, 6, 8, 13), so the frame would show it.
POS16 = (3, 8, 5, 13, 7, 0, 8, 2, 13, 6, 0, 7, 1, 13, 4, 3)
ROPE_POS16 = (0, 1, 2999, 17, 1024, 3000, 511, 77, 2048, 5, 1500, 333, 2500, 64, 999, 12)


def _grid(ns, cols, ks):
    """Every (n, N) pair, the K values rotating so that each meets every n and every N position; K <= 1088 where N >= 4100."""
    out = []
    for (i, n), (j, N) in itertools.product(enumerate(ns), enumerate(cols)):
        small = [k for k in ks if k <= 1088] if N >= 4100 else list(ks)
        out.append((n, N, small[(i + j) % len(small)]))
    return out


PLAIN_SHAPES = _grid(NS_ROWS, NS_COLS, KS) + [(16, 8200, 3136)]
QKV_CASES = [(h, n, QKV_KS[(i + j) % 3], bool((i + j) % 6 // 3)) for (i, h), (j, n) in itertools.product(enumerate(HEADS), enumerate(NS_ROWS))]
W4_SHAPES = [(n, N, (128, 384)[(i + j) % 2]) for (i, n), (j, N) in itertools.product(enumerate((1, 8, 9, 16)), enumerate((4, 20, 37)))] + [(16, 4112, 1152)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _sync():
    """Wait for the launch; a fault of the device ends the session there, so that nothing more is launched on it."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU faulted, nothing more is launched: {e}", returncode=3)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


class _Problem:
    """16 activation rows, W (and W2), bias and 16 residual rows, drawn once; the fp64 products of all 16 rows.  Every call frames its own rows."""
    def __init__(self, N, K, seed, w2=False):
        self.N, self.K = N, K
        self.x16 = _rand((16, K), 1000 + seed)
        w = _rand((N, K), 2000 + seed, K ** -0.5)
        self.w = framed_operand(w, 0, G)
        self.bias = framed_operand(_rand((N,), 3000 + seed), 0, G)
        self.res16 = _rand((16, N), 4000 + seed)
        xd = self.x16.double()
        self.core, self.core_abs = xd @ w.double().t(), xd.abs() @ w.double().abs().t()
        if w2:
            w_up = _rand((N, K), 5000 + seed, K ** -0.5)
            self.w2 = framed_operand(w_up, 0, G)
            self.core2, self.core2_abs = xd @ w_up.double().t(), xd.abs() @ w_up.double().abs().t()

    def x(self, rows):
        return framed_operand(self.x16[rows], 8, G)


def _plain_call(ops, prob, rows, e):
    """One launch of mode 0 on the rows `rows` of the problem with epilogue e -> {name: (view of 16 rows, frame check)}."""
    n, N = len(range(*rows.indices(16))), prob.N
    use_bias, use_res = "bias" in e or e in ("f32", "both"), "residual" in e or e in ("inplace", "both")
    res = framed_operand(prob.res16[rows], 8, G) if use_res and e != "inplace" else None
    outs = {}
    if e != "f32":
        outs["bf16"] = framed_out_rows(n, N, 8, G, fill=prob.res16[rows] if e == "inplace" else None)
    if e in ("f32", "both"):
        outs["f32"] = framed_out_rows(n, N, 8, G, dtype=torch.float32)
    y = outs["bf16"][0] if "bf16" in outs else None
    ops.gemm_batch(prob.x(rows), prob.w, bias=prob.bias if use_bias else None, residual=y if e == "inplace" else res, out=y,
                   out_f32=outs["f32"][0] if "f32" in outs else None)
    _sync()
    return outs


def _plain_refs(prob, rows, e):
    use_bias, use_res = "bias" in e or e in ("f32", "both"), "residual" in e or e in ("inplace", "both")
    b, r = prob.bias.double() if use_bias else None, prob.res16[rows].double() if use_res else None
    return {"bf16": bgemm_plain_bound(prob.core[rows], prob.core_abs[rows], prob.K, b, r), "f32": bgemm_plain_bound(prob.core[rows], prob.core_abs[rows], prob.K, b, out_f32=True)}


@pytest.mark.parametrize("n,N,K", PLAIN_SHAPES, ids=str)
def test_plain_every_epilogue(ops, n, N, K):
    prob = _Problem(N, K, seed=n + N + K)
    rows = slice(0, n)
    worst = 0.0
    for e in EPILOGUES:
        what = f"plain ({n}, {N}, {K}) [{e}]"
        outs, refs = _plain_call(ops, prob, rows, e), _plain_refs(prob, rows, e)
        for name, (view, check) in outs.items():
            worst = max(worst, assert_elementwise(view[:n], *refs[name], f"{what} {name}"))
            check()
        again = _plain_call(ops, prob, rows, e)
        for name in outs:
            assert torch.equal(_bits(outs[name][0][:n]), _bits(again[name][0][:n])), f"{what} {name}: two calls differ"
        full = _plain_call(ops, prob, slice(0, 16), e)
        for name in outs:
            assert torch.equal(_bits(outs[name][0][:n]), _bits(full[name][0][:n])), f"{what} {name}: rows differ from those of the 16-row call"
            full[name][1]()
        if e in INDEPENDENCE_EPILOGUES:
            for m in range(n):
                solo = _plain_call(ops, prob, slice(m, m + 1), e)
                for name in outs:
                    assert torch.equal(_bits(outs[name][0][m]), _bits(solo[name][0][0])), f"{what} {name}: row {m} differs from the row computed alone"
                    solo[name][1]()
    print(f"plain ({n}, {N}, {K}): worst err / bound {worst:.3f}")


def _gateup_call(ops, prob, rows):
    n = len(range(*rows.indices(16)))
    view, check = framed_out_rows(n, prob.N, 8, G)
    ops.gemm_batch(prob.x(rows), prob.w, w2=prob.w2, out=view)
    _sync()
    return view, check


@pytest.mark.parametrize("n,N,K", PLAIN_SHAPES, ids=str)
def test_gateup(ops, n, N, K):
    prob = _Problem(N, K, seed=n + N + K + 1, w2=True)
    what = f"gate/up ({n}, {N}, {K})"
    view, check = _gateup_call(ops, prob, slice(0, n))
    ref, bound = bgemm_gateup_bound(prob.core[:n], prob.core_abs[:n], prob.core2[:n], prob.core2_abs[:n], K)
    worst = assert_elementwise(view[:n], ref, bound, what)
    check()
    assert torch.equal(_bits(view[:n]), _bits(_gateup_call(ops, prob, slice(0, n))[0][:n])), f"{what}: two calls differ"
    full, check16 = _gateup_call(ops, prob, slice(0, 16))
    assert torch.equal(_bits(view[:n]), _bits(full[:n])), f"{what}: rows differ from those of the 16-row call"
    check16()
    for m in range(n):
        solo, check1 = _gateup_call(ops, prob, slice(m, m + 1))
        assert torch.equal(_bits(view[m]), _bits(solo[0])), f"{what}: row {m} differs from the row computed alone"
        check1()
    print(f"{what}: worst err / bound {worst:.3f}")


# ---- q|k|v ----------------------------------------------------------------------------------------------------------------------------------------------
def _qkv_call(ops, prob, heads, rows, use_bias, cs16):
    nq, nkv, hd = heads
    idx = list(range(*rows.indices(16)))
    n = len(idx)
    q, check_q = framed_out_rows(n, nq * hd, 8, G)
    kc, check_k = framed_cache(nkv, MAX_CTX, hd)
    vc, check_v = framed_cache(nkv, MAX_CTX, hd)
    pos = [POS16[m] for m in idx]
    pos_t = framed_operand(torch.tensor(pos, dtype=torch.int32, device="cuda"), 0, 1, pad=MAX_CTX - 1)     # (int32: a neighbour's position, not NaN)
    cs = framed_operand(cs16[rows].reshape(-1), 0, G).view(n, hd)
    ops.qkv_batch(prob.x(rows), prob.w, prob.bias if use_bias else None, q, kc, vc, pos_t, cs, nq, nkv, hd)
    _sync()
    return q, kc, vc, pos, (check_q, check_k, check_v)


@pytest.mark.parametrize("heads,n,K,use_bias", QKV_CASES, ids=str)
def test_qkv_rope_and_cache_rows(ops, heads, n, K, use_bias):
    nq, nkv, hd = heads
    N = (nq + 2 * nkv) * hd
    prob = _Problem(N, K, seed=n + N + K + 2)
    cs16 = rope_table(ROPE_POS16, hd, device="cuda")
    what = f"qkv {heads} n={n} K={K} bias={use_bias}"
    rows = slice(0, n)
    q, kc, vc, pos, checks = _qkv_call(ops, prob, heads, rows, use_bias, cs16)
    ref, bound = bgemm_qkv_bound(prob.core[:n], prob.core_abs[:n], K, prob.bias.double() if use_bias else None, cs16[:n].double(), nq, nkv, hd)
    worst = assert_qkv_outputs(q, kc, vc, checks, pos, n, ref, bound, nq, nkv, hd, what)
    q2, kc2, vc2, _, _ = _qkv_call(ops, prob, heads, rows, use_bias, cs16)
    assert torch.equal(_bits(q[:n]), _bits(q2[:n])) and torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2)), f"{what}: two calls differ"
    qf, kcf, vcf, _, checks16 = _qkv_call(ops, prob, heads, slice(0, 16), use_bias, cs16)
    assert torch.equal(_bits(q[:n]), _bits(qf[:n])) and torch.equal(_bits(kc[:n]), _bits(kcf[:n])) and torch.equal(_bits(vc[:n]), _bits(vcf[:n])), \
        f"{what}: rows differ from those of the 16-row call"
    checks16[0](); checks16[1](POS16, 16); checks16[2](POS16, 16)
    for m in range(n):
        q1, kc1, vc1, _, checks1 = _qkv_call(ops, prob, heads, slice(m, m + 1), use_bias, cs16)
        assert torch.equal(_bits(q[m]), _bits(q1[0])) and torch.equal(_bits(kc[m]), _bits(kc1[0])) and torch.equal(_bits(vc[m]), _bits(vc1[0])), \
            f"{what}: row {m} differs from the row computed alone"
        checks1[0](); checks1[1](POS16[m:m + 1], 1); checks1[2](POS16[m:m + 1], 1)
    print(f"{what}: worst err / bound {worst:.3f}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(ops):
    """n = 0 and 17, K = 96, ldx % 8 != 0, head_dim 48, a NULL output: each raises with launch_bgemm's (or the entry's) message, leaves the output
    untouched, and a correct call afterwards still passes."""
    from vila_amd import _lib
    lib = _lib.load()
    N, K = 20, 64
    prob = _Problem(N, K, seed=5)
    x17 = framed_operand(_rand((17, K), 6), 8, G)
    out, check = framed_out_rows(0, N, 8, G, rows=17)
    for n, pat in ((0, "1..16"), (17, "1..16")):
        with pytest.raises(ValueError, match=pat):
            ops.gemm_batch(x17, prob.w, out=out, n=n)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.gemm_batch(framed_operand(_rand((2, 96), 7), 8, G), framed_operand(_rand((N, 96), 8), 0, G), out=out)
    with pytest.raises(ValueError, match="alignment"):
        ops.gemm_batch(framed_operand(_rand((2, K), 9), 4, G), prob.w, out=out)
    s = torch.cuda.current_stream().cuda_stream
    x2 = prob.x(slice(0, 2))
    assert lib.vila_gemm_batch_bf16(x2.data_ptr(), x2.stride(0), 2, prob.w.data_ptr(), None, None, None, 0, None, 0, None, 0, N, K, s) == -1
    assert "NULL output" in lib.vila_last_error().decode()
    nq, nkv, hd = 2, 1, 48
    q, check_q = framed_out_rows(0, nq * hd, 8, G)
    kc, check_k = framed_cache(nkv, MAX_CTX, hd)
    vc, check_v = framed_cache(nkv, MAX_CTX, hd)
    pos = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="head_dim"):
        ops.qkv_batch(x2, framed_operand(_rand(((nq + 2 * nkv) * hd, K), 10), 0, G), None, q, kc, vc, pos, rope_table(ROPE_POS16, hd, device="cuda"), nq, nkv, hd)
    assert lib.vila_qkv_batch_bf16(x2.data_ptr(), x2.stride(0), 2, prob.w.data_ptr(), None, None, q.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0),
                                   pos.data_ptr(), pos.data_ptr(), 2, 1, 32, MAX_CTX, K, s) == -1
    assert "NULL" in lib.vila_last_error().decode()
    _sync()
    check(); check_q(); check_k([], 0); check_v([], 0)
    outs, refs = _plain_call(ops, prob, slice(0, 2), "bias+residual"), _plain_refs(prob, slice(0, 2), "bias+residual")
    assert_elementwise(outs["bf16"][0][:2], *refs["bf16"], "the correct call after the refusals")
    outs["bf16"][1]()


# ---- the W4A16 sibling through the same frames -------------------------------------------------------------------------------------------------------------
def _rows_cols_rel_l2(out, ref, what, tol):
    """tests/test_gpu_gemm_elements.py::_rows_cols_rel_l2: every single row and every single column within tol."""
    o = out.double()
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite elements at {(~torch.isfinite(o)).nonzero()[:8].tolist()}"
    d = o - ref
    worst = []
    for dim, name in ((1, "row"), (0, "column")):
        rel = d.norm(dim=dim) / ref.norm(dim=dim).clamp_min(1e-30)
        i = int(rel.argmax())
        assert float(rel[i]) < tol, f"{what}: {name} {i} rel-L2 {float(rel[i]):.3e} (bound {tol:g}); {int((rel >= tol).sum())} {name}s over it"
        worst.append(float(rel[i]))
    return worst


@pytest.mark.parametrize("kind", ["plain", "gateup"])
@pytest.mark.parametrize("n,N,K", W4_SHAPES, ids=str)
def test_w4_batch_sibling_in_frames(ops, n, N, K, kind):
    """At n = 1 a column's rel-L2 is one element's relative error, which no kernel keeps small where the element is a difference of larger
    terms.  The inputs therefore keep every element away from zero.  Gate/up: weights and activations with a mean (x ~ 1 + N(0, 1),
    w ~ 0.02 (0.5 + N(0, 1)): gate and up are 0.01 K +- 0.03 sqrt(K), never near zero).  Plain: zero-mean weights, so that x . w + bias is
    N(0, 0.0008 K + 0.25), at most 1.1^2 here, and a residual of magnitude 8 + |N(0, 1)| with a random sign: the projection's own rounding (2^-8
    of ITS size, decode_batch.hip:103 mirrored by gemv_w4_batch.hip:119) stays below 2^-8 of the result while |x . w + bias| < 4, and the result's
    relative error below 2 * 2^-8 < 1e-2.  The frames and the indexing see the same kernel either way.  Every element is also held to
    w4_generic_bound, which needs no such care: it is absolute where the element is a difference of larger terms."""
    from vila_amd.quant import W4Matrix
    g = torch.Generator(device="cuda").manual_seed(n + N + K)
    draw = lambda mean: (mean + torch.randn((N, K), generator=g, device="cuda")) * 0.02
    mat = W4Matrix.pack(draw(0.5), draw(0.5)) if kind == "gateup" else W4Matrix.pack(draw(0.0))
    x = framed_operand((1.0 + torch.randn((n, K), generator=g, device="cuda")).to(torch.bfloat16), 8, G)
    what = f"w4 batch {kind} ({n}, {N}, {K})"
    if kind == "gateup":
        wg, wu = mat.dequantized()
        bias = res = None
        ref, tol = torch.nn.functional.silu(x.double() @ wg.double().t()) * (x.double() @ wu.double().t()), 1.5e-2
    else:
        bias = framed_operand((torch.randn((N,), generator=g, device="cuda") * 0.5).to(torch.bfloat16), 0, G)
        r = torch.randn((n, N), generator=g, device="cuda")
        res = framed_operand((torch.sign(r) * (8.0 + r.abs())).to(torch.bfloat16), 0, G)
        ref, tol = x.double() @ mat.dequantized().double().t() + bias.double() + res.double(), 1e-2
    out, check = framed_out_rows(n, N, 0, G)
    ops.gemv_w4_batch(x, mat, bias=bias, residual=res, out=out)
    _sync()
    q, z, s = w4_unpack(mat.logical)
    if kind == "gateup":
        (cg, ag), (cu, au) = w4_generic_acc(x.double(), q[0::2], z[0::2], s[0::2]), w4_generic_acc(x.double(), q[1::2], z[1::2], s[1::2])
        worst = assert_elementwise(out[:n], *w4_generic_bound("gateup", K, cg, ag, cu, au), what)
    else:
        core, acc = w4_generic_acc(x.double(), q, z, s)
        worst = assert_elementwise(out[:n], *w4_generic_bound("plain", K, core, acc, bias64=bias.double(), res64=res.double()), what)
    r, c = _rows_cols_rel_l2(out[:n], ref, what, tol)
    check()
    out2, _ = framed_out_rows(n, N, 0, G)
    ops.gemv_w4_batch(x, mat, bias=bias, residual=res, out=out2)
    _sync()
    assert torch.equal(_bits(out[:n]), _bits(out2[:n])), f"{what}: two calls differ"
    print(f"{what}: worst err / bound {worst:.3f}, worst row {r:.2e}, worst column {c:.2e}")

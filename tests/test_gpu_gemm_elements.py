"""Every element of every GEMM family's output against a derived bound, inside framed buffers.

The other GEMM tests judge an output by one number, the rel-L2 of the whole matrix (< 4e-3 against a floor of 1.66e-3): a fault confined to one
tile edge fits inside it (tests/test_gemm_bound_cpu.py shows which ones).  Here each case
  - builds A, W, bias and residual as views of larger buffers whose padding columns and guard rows are NaN (lda = K + 8, ldw = K + 8, ldr = N + 4):
    a read outside an operand that reaches the result shows in it;
  - writes into a view (ldc = N + 8, guard rows on both sides) of a buffer holding a bit pattern, and into a workspace of exactly the bytes the
    entry point was told, with patterned guards: a store outside the output or past the workspace shows in the frame;
  - asserts from vila_gemm_plan_describe, under the same hooks, that the launch is the family the case names;
  - checks every element against gemm_elem_bound (tests/gpu_util.py) with an fp64 reference of the same bf16 inputs.

roundings = 1 for every bf16 family: bias and residual are added in fp32 and the sum is rounded once — gemm.hip:183-188 (register-staged kernels),
gemm_ring.hip:258 (rings), gemm256_kernel.h:744 / 776 / 815 (256x256 kernel, all layouts), gemm256.hip:59-68 (split-K reduce), gemm256.hip:221-230
(tail reduce), gemm_ring_splitk.hip:179 (ring reduce), gemm_i8.hip:160-169 (W8A8).  roundings = 0 for the fp32 output (gemm.hip:186: stored as summed).

Shapes are the smallest that straddle each family's tile (BM x BN, K-tile 64): M in {1, BM - 1, BM + 1, 2 BM + 16}, N in {4, BN - 4, BN + 4},
K in {the family's minimum, 64 + 8, an odd number of K-tiles + 8}, K <= 1500 so that the accumulation term of the bound stays below its rounding
term; one K = 4304 case per K-sliced family.  Shape constraints that drop combinations: the 256x256 kernel needs K >= 128, the rings K >= 64, a
K-sliced launch at least 15 K-tiles (two slices of 8), the forward split-K M >= 512 below 128 K-tiles, a contraction-major operand rows % 8 == 0,
the W8A8 kernel K >= 128 and K % 16 == 0."""
import ctypes
import itertools

import pytest
import torch

from tests.gpu_util import assert_elementwise, framed_operand, framed_out, framed_ws, gemm_elem_bound

pytestmark = pytest.mark.gpu

G = 4                                                    # guard rows on each side of every framed operand and output
KNOB_DEFAULTS = {"tile": 0, "sched": 0, "hybrid": 1, "bm": 0, "ex": -1, "group": -1}
EPILOGUES = ("none", "bias", "residual", "bias+residual", "inplace")


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


def _grid(ms, ns, ks):
    """Every (M, N) pair, the K values rotating so that each meets every M and every N position."""
    return [(m, n, ks[(i + j) % len(ks)]) for (i, m), (j, n) in itertools.product(enumerate(ms), enumerate(ns))]


class _Knobs:
    """The tuning hooks of include/vila_hip_tuning.h for one case: set on entry, always reset on exit."""
    def __init__(self, **knobs):
        from vila_amd import _lib
        self.lib, self.knobs = _lib.load(), knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            getattr(self.lib, "vila_gemm_force_" + k)(v)
        return self

    def __exit__(self, *exc):
        for k in self.knobs:
            getattr(self.lib, "vila_gemm_force_" + k)(KNOB_DEFAULTS[k])

    def plan(self, M, N, K, epi=0, out_f32=0, a_cm=0, b_cm=0, ws_bytes=0):
        buf = ctypes.create_string_buffer(256)
        assert self.lib.vila_gemm_plan_describe(M, N, K, epi, out_f32, a_cm, b_cm, ws_bytes, 0, buf, len(buf)) > 0
        return dict(kv.split("=") for kv in buf.value.decode().split())

    def expect(self, want, ws_bytes=0, **shape):
        """The plan under these hooks must be the launch the case intends: a force hook that fell back to another kernel fails here.  `want` maps
        describe's fields to a value, or to a predicate for counts that follow from the shape (splits)."""
        got = self.plan(ws_bytes=ws_bytes, **shape)
        for k, v in want.items():
            ok = v(int(got[k])) if callable(v) else str(got[k]) == str(v)
            assert ok, f"{shape}: the plan is {got}, the case wants {k}={v if not callable(v) else '<predicate>'}"
        if int(got["splits"]) > 1 and got["family"] in ("256_sliced", "cm_sliced", "ring_splitk"):
            assert int(got["splits"]) * shape["M"] * shape["N"] * 4 <= ws_bytes, (got, ws_bytes)
        return got


class _Problem:
    """Framed operands of C[M, N] = A . B^T (+ bias) (+ residual) and its fp64 reference.  a_cm / b_cm: that operand is stored [K][rows]."""
    def __init__(self, M, N, K, a_cm=False, b_cm=False, seed=0, w2=False):
        self.M, self.N, self.K = M, N, K
        a = _rand((K, M) if a_cm else (M, K), 1000 + seed)
        w = _rand((K, N) if b_cm else (N, K), 2000 + seed, K ** -0.5)
        self.a, self.w = framed_operand(a, 8, G), framed_operand(w, 8, G)
        self.bias = framed_operand(_rand((N,), 3000 + seed), 0, G)
        self.res = framed_operand(_rand((M, N), 4000 + seed), 4, G)
        ad, wd = (a.double().t() if a_cm else a.double()), (w.double() if b_cm else w.double().t())
        self.core, self.core_abs = ad @ wd, ad.abs() @ wd.abs()
        if w2:
            w_up = _rand((N, K), 5000 + seed, K ** -0.5)
            self.w2 = framed_operand(w_up, 8, G)
            self.core2 = ad @ w_up.double().t()

    def ref(self, bias, residual):
        r, p = self.core.clone(), self.core_abs.clone()
        if bias:
            r += self.bias.double(); p += self.bias.double().abs()
        if residual:
            r += self.res.double(); p += self.res.double().abs()
        return r, p


def _run_epilogues(call, prob, what, ws_bytes=0, out_f32=False, epilogues=EPILOGUES, roundings=1):
    """call(bias, residual, out, ws) launches the GEMM.  Every epilogue: framed output (for the in-place form the residual's own frame), framed
    workspace, every element against the bound, every frame intact."""
    M, N, K = prob.M, prob.N, prob.K
    worst = 0.0
    for e in epilogues:
        use_bias, use_res = "bias" in e, "residual" in e or e == "inplace"
        ref, absprod = prob.ref(use_bias, use_res)
        out, check_out = framed_out(M, N, 8, G, torch.float32 if out_f32 else torch.bfloat16, fill=prob.res if e == "inplace" else None)
        ws, check_ws = framed_ws(ws_bytes) if ws_bytes else (None, lambda: None)
        call(prob.bias if use_bias else None, out if e == "inplace" else prob.res if use_res else None, out, ws)
        _sync()
        bound = gemm_elem_bound(ref, absprod, K, roundings=0 if out_f32 else roundings)
        worst = max(worst, assert_elementwise(out, ref, bound, f"{what} [{e}]"))
        check_out(); check_ws()
    print(f"{what}: worst err / bound {worst:.3f}")


def _forward(ops, M, N, K, knobs, want, ws_slices=0, **kw):
    # roundings = 1 (the default of _run_epilogues) for every forward family: fp32 bias and residual adds, one pack2bf — gemm.hip:183-188,
    # gemm_ring.hip:258, gemm256_kernel.h:744 / 776 / 815, and the reduces gemm256.hip:68, gemm256.hip:230, gemm_ring_splitk.hip:179; 0 for out_f32
    ws_bytes = ws_slices * M * N * 4
    with _Knobs(**knobs) as k:
        k.expect(want, ws_bytes=ws_bytes, M=M, N=N, K=K, out_f32=int(kw.get("out_f32", False)))
        prob = _Problem(M, N, K, seed=M + N + K)
        _run_epilogues(lambda b, r, o, ws: ops.gemm(prob.a, prob.w, bias=b, residual=r, out=o, out_f32=kw.get("out_f32", False), ws=ws), prob,
                       f"{want.get('family')} {knobs} ({M}, {N}, {K})", ws_bytes=ws_bytes, **kw)


# ---- forward bf16, one forced tile each --------------------------------------------------------------------------------------------------------------
# tile hook -> (family, ring, pipe, BM, BN, K values): gemm_plan.h gemm_plan().  Rings need K >= 64 (gemm_ring_supported).
REG_K, RING_K, K256 = (8, 72, 200), (64, 72, 200), (128, 136, 328)
FORCED_TILES = {
    1: ("reg128x128", 0, 0, 128, 128, REG_K), 2: ("reg128x64", 0, 0, 128, 64, REG_K), 3: ("reg256x128", 0, 0, 256, 128, REG_K),
    7: ("ring", 3, 2, 128, 64, RING_K), 6: ("ring", 4, 2, 128, 64, RING_K), 8: ("ring", 8, 2, 128, 128, RING_K),
    12: ("ring", 3, 2, 128, 64, RING_K), 13: ("ring", 8, 2, 128, 128, RING_K), 14: ("ring", 4, 2, 128, 64, RING_K),
    15: ("ring", 3, 0, 128, 64, RING_K), 16: ("ring", 8, 0, 128, 128, RING_K), 17: ("ring", 4, 0, 128, 64, RING_K),
}


def _tile_shapes(bm, bn, ks):
    return _grid((1, bm - 1, bm + 1, 2 * bm + 16), (4, bn - 4, bn + 4), ks)


FORWARD_CASES = [(t, s) for t, (_, _, _, bm, bn, ks) in FORCED_TILES.items() for s in _tile_shapes(bm, bn, ks)]
SHAPES_256 = _tile_shapes(256, 256, K256)
# K-sliced launches need 15 K-tiles for two slices of 8: K = 15 tiles + 8, 16 tiles + 8, 23 tiles + 8, and one long contraction
SLICED_K = (968, 1032, 1480)
SPLITK_SHAPES = _grid((513, 528, 600), (4, 252, 260), SLICED_K) + [(600, 260, 4304)]
RING_SPLITK_SHAPES = _grid((1, 127, 129, 272), (4, 60, 68), SLICED_K) + [(129, 68, 4304)]
# more than 256 tiles of 256^2 with a short last round: 17 x 16 tiles, ragged last row tile and last column tile, 16 K-tiles + 8; and the long K
HYBRID_SHAPES = [(4300, 4092, 1032), (4300, 4092, 4304)]
EX_SHAPES = [(257, 260, 136), (272, 252, 328), (513, 4, 128), (528, 260, 200)]
W8A8_SHAPES = _grid((1, 127, 129, 272), (4, 60, 68), (128, 144, 272))

# every (M, N, K) a forward case runs: tests/test_gemm_bound_cpu.py shows the once-rounded fp32 reference inside the bound at each
ALL_FORWARD_SHAPES = sorted({s for _, s in FORWARD_CASES} | set(SHAPES_256) | set(_tile_shapes(192, 256, K256)) | set(SPLITK_SHAPES) | set(RING_SPLITK_SHAPES) |
                            set(HYBRID_SHAPES) | set(EX_SHAPES))


@pytest.mark.parametrize("tile,shape", FORWARD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forward_forced_tile(ops, tile, shape):
    """vila_gemm_force_tile 1 / 2 / 3 (register-staged), 6 / 7 / 8 and 12 - 17 (LDS-DMA rings, PIPE 2 and plain)."""
    fam, ring, pipe, _, _, _ = FORCED_TILES[tile]
    _forward(ops, *shape, dict(tile=tile), dict(family=fam, ring=ring, pipe=pipe))


@pytest.mark.parametrize("shape", SHAPES_256, ids=str)
@pytest.mark.parametrize("sched", [0, 1, 2, 3, 5, 6, 10])
def test_forward_256_every_schedule(ops, sched, shape):
    """vila_gemm_force_tile(4): the 256x256 LDS-DMA kernel with its default and every kept K-loop schedule."""
    _forward(ops, *shape, dict(tile=4, sched=sched), dict(family="256", sched=sched, ex=0))


@pytest.mark.parametrize("bm,shape", [(bm, s) for bm in (192, 256) for s in _tile_shapes(bm, 256, K256)], ids=str)
def test_forward_256_tile_height(ops, bm, shape):
    _forward(ops, *shape, dict(tile=4, bm=bm), dict(family="256", bm=bm))


@pytest.mark.parametrize("shape", EX_SHAPES, ids=str)
def test_forward_256_leftover_fragment(ops, shape):
    """M = 256 k + r, r in {1, 16}: the rows ride in the last row tile as an extra fragment (vila_gemm_force_ex(2))."""
    _forward(ops, *shape, dict(tile=4, ex=2, bm=256), dict(family="256", ex=1))


@pytest.mark.parametrize("shape", SPLITK_SHAPES, ids=str)
def test_forward_splitk_workspace(ops, shape):
    """vila_gemm_force_tile(5): K-sliced 256x256 slabs + reduce.  The workspace holds three slices: where the plan would take more (K = 4304) the
    split count must follow ws_bytes, and the slabs must end where the workspace does."""
    _forward(ops, *shape, dict(tile=5), dict(family="256_sliced", splits=lambda s: 2 <= s <= 3, reduce="plain"), ws_slices=3)


@pytest.mark.parametrize("shape", RING_SPLITK_SHAPES, ids=str)
def test_forward_ring_splitk_workspace(ops, shape):
    """vila_gemm_force_tile(11): the K-sliced 128x64 ring, three slices' worth of workspace (the plan's cap is four)."""
    _forward(ops, *shape, dict(tile=11), dict(family="ring_splitk", splits=lambda s: 2 <= s <= 3, reduce="plain"), ws_slices=3)


@pytest.mark.parametrize("shape", HYBRID_SHAPES, ids=str)
def test_forward_hybrid_rounds_plus_sliced_tail(ops, shape):
    """Whole rounds + K-sliced tail tiles (vila_gemm_force_hybrid(1)): 272 tiles = 256 + 16; the workspace holds exactly five slices of the 16
    compact tail slabs (the plan takes three at K = 1032, and five of the eight it would like at K = 4304)."""
    M, N, K = shape
    ws_bytes = 5 * 16 * 65536 * 4
    with _Knobs(hybrid=1) as k:
        got = k.expect(dict(family="256_hybrid", tail=16, full=256, splits=lambda s: 2 <= s <= 5, reduce="tail"), ws_bytes=ws_bytes, M=M, N=N, K=K)
        assert (K == 4304) == (int(got["splits"]) == 5), got
        prob = _Problem(M, N, K, seed=7)
        _run_epilogues(lambda b, r, o, ws: ops.gemm(prob.a, prob.w, bias=b, residual=r, out=o, ws=ws), prob, f"256_hybrid {shape}", ws_bytes=ws_bytes)


@pytest.mark.parametrize("tile,shape", [(t, s) for t, bm, bn, ks in ((1, 128, 128, REG_K), (2, 128, 64, REG_K), (3, 256, 128, REG_K), (4, 256, 256, K256))
                                        for s in _tile_shapes(bm, bn, ks)], ids=str)
def test_forward_fp32_output(ops, tile, shape):
    """out_f32 of the families that have it (the rings and the K-sliced launches refuse it): no bf16 term in the bound (roundings = 0)."""
    fam = {1: "reg128x128", 2: "reg128x64", 3: "reg256x128", 4: "256"}[tile]
    _forward(ops, *shape, dict(tile=tile), dict(family=fam), out_f32=True, epilogues=("none", "bias+residual"))


# ---- contraction-major operands (vila_gemm_bf16_t) ----------------------------------------------------------------------------------------------------
# dgrad: B stored [K][N] (N % 8, K % 8 for the row-major A); wgrad: both stored [K][rows] (rows % 8, any K: 777, 333); a_cm only: K % 8, N % 4
CM_LAYOUTS = {"dgrad": (False, True), "wgrad": (True, True), "a_cm": (True, False)}
CM_SHAPES = {
    "dgrad": _grid((1, 255, 257, 528), (8, 248, 264), K256),
    "wgrad": _grid((8, 248, 264, 528), (8, 248, 264), (128, 333, 777)),
    "a_cm": _grid((8, 248, 264, 528), (4, 252, 260), K256),
}
CM_SLICED_SHAPES = {
    "dgrad": _grid((1, 257, 528), (8, 264), SLICED_K) + [(257, 264, 4304)],
    "wgrad": _grid((8, 264, 528), (8, 264), (961, 1033, 1481)) + [(264, 264, 4301)],
    "a_cm": _grid((8, 264, 528), (4, 260), SLICED_K) + [(264, 260, 4304)],
}


def _gemm_t(ops, layout, M, N, K, want, ws_bytes=0, seed=0):
    a_cm, b_cm = CM_LAYOUTS[layout]
    with _Knobs(hybrid=1) as k:
        got = k.expect(want, ws_bytes=ws_bytes, M=M, N=N, K=K, a_cm=int(a_cm), b_cm=int(b_cm))
        prob = _Problem(M, N, K, a_cm=a_cm, b_cm=b_cm, seed=M + N + K + seed)
        # roundings = 1: the contraction-major layouts share the 256x256 kernel's epilogue (gemm256_kernel.h:744 / 776 / 815) and the reduces
        # (gemm256.hip:68 split-K, gemm256.hip:230 tail): fp32 adds, rounded once
        _run_epilogues(lambda b, r, o, ws: ops.gemm_t(prob.a, prob.w, a_cm=a_cm, b_cm=b_cm, bias=b, residual=r, out=o, ws=ws), prob,
                       f"{got['family']} {layout} ({M}, {N}, {K})", ws_bytes=ws_bytes)


@pytest.mark.parametrize("layout,shape", [(l, s) for l, ss in CM_SHAPES.items() for s in ss], ids=str)
def test_gemm_t_whole(ops, layout, shape):
    _gemm_t(ops, layout, *shape, dict(family="cm", splits=1))


@pytest.mark.parametrize("layout,shape", [(l, s) for l, ss in CM_SLICED_SHAPES.items() for s in ss], ids=str)
def test_gemm_t_sliced_workspace(ops, layout, shape):
    """With a workspace of three slices an under-filled grid is K-sliced (cm_sliced); the split count follows ws_bytes at the long contraction."""
    M, N, K = shape
    _gemm_t(ops, layout, M, N, K, dict(family="cm_sliced", splits=lambda s: 2 <= s <= 3, reduce="plain"), ws_bytes=3 * M * N * 4)


@pytest.mark.parametrize("layout,shape", [("wgrad", (4296, 4088, 1097)), ("dgrad", (4300, 4088, 1032))], ids=str)
def test_gemm_t_hybrid_rounds_plus_sliced_tail(ops, layout, shape):
    """17 x 16 tiles with a contraction-major operand: whole rounds + 16 K-sliced tail tiles, workspace of exactly the two slices the plan takes."""
    _gemm_t(ops, layout, *shape, dict(family="cm_hybrid", tail=16, full=256, splits=2, reduce="tail"), ws_bytes=2 * 16 * 65536 * 4)


# ---- GELU and gate/up epilogues: finite, frame intact, every single row and column within the project's tolerance for the epilogue -------------------
def _rows_cols_rel_l2(out, ref, what, tol=5e-3):
    o = out.double()
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite elements at {(~torch.isfinite(o)).nonzero()[:8].tolist()}"
    d = o - ref
    for dim, name in ((1, "row"), (0, "column")):
        rel = d.norm(dim=dim) / ref.norm(dim=dim).clamp_min(1e-30)
        i = int(rel.argmax())
        assert float(rel[i]) < tol, f"{what}: {name} {i} rel-L2 {float(rel[i]):.3e} (bound {tol:g}); {int((rel >= tol).sum())} {name}s over it"
    return float((d.norm(dim=1) / ref.norm(dim=1)).max()), float((d.norm(dim=0) / ref.norm(dim=0)).max())


def _act_shapes(bm, bn, ks):
    return _grid((max(64, bm - 1), bm + 1, 2 * bm + 16), (max(64, bn - 4), bn + 4), ks)


GELU_TILES = {1: ("reg128x128", 128, 128, (8, 72, 200)), 2: ("reg128x64", 128, 64, (8, 72, 200)), 3: ("reg256x128", 256, 128, (8, 72, 200)),
              4: ("256", 256, 256, K256), 12: ("ring", 128, 64, RING_K), 13: ("ring", 128, 128, RING_K), 14: ("ring", 128, 64, RING_K),
              15: ("ring", 128, 64, RING_K), 16: ("ring", 128, 128, RING_K), 17: ("ring", 128, 64, RING_K)}


@pytest.mark.parametrize("epi", [1, 2], ids=["tanh", "erf"])
@pytest.mark.parametrize("tile,shape", [(t, s) for t, (_, bm, bn, ks) in GELU_TILES.items() for s in _act_shapes(bm, bn, ks)], ids=str)
def test_gelu_epilogues_every_row_and_column(ops, tile, shape, epi):
    M, N, K = shape
    fn = (lambda t: torch.nn.functional.gelu(t, approximate="tanh")) if epi == 1 else torch.nn.functional.gelu
    with _Knobs(tile=tile) as k:
        k.expect(dict(family=GELU_TILES[tile][0]), M=M, N=N, K=K, epi=epi)
        prob = _Problem(M, N, K, seed=M + N + K + epi)
        out, check = framed_out(M, N, 8, G)
        ops.gemm(prob.a, prob.w, bias=prob.bias, epi=epi, out=out)
        _sync()
    r, c = _rows_cols_rel_l2(out, fn(prob.core + prob.bias.double()), f"gelu epi={epi} tile={tile} {shape}")
    check()
    print(f"gelu epi={epi} tile={tile} {shape}: worst row {r:.2e}, worst column {c:.2e}")


GATEUP_CASES = [(t, s, 0) for t, bm, bn, ks in ((1, 128, 64, REG_K), (3, 256, 64, REG_K), (4, 256, 128, K256)) for s in _act_shapes(bm, bn, ks)]
GATEUP_CASES.append((4, (4300, 2044, 1032), 4))      # 17 x 16 tiles of 256 x 128: whole rounds fused + the last tile column K-sliced four ways


@pytest.mark.parametrize("tile,shape,ws_slices", GATEUP_CASES, ids=str)
def test_gateup_every_row_and_column(ops, tile, shape, ws_slices):
    M, N, K = shape
    ws_bytes = ws_slices * 2 * M * 124 * 4                # the tail's 124 columns, gate and up planes
    want = dict(family="256_hybrid", reduce="gateup", splits=4, tail=17) if ws_slices else dict(family={1: "reg128x128", 3: "reg256x128", 4: "256"}[tile])
    with _Knobs(tile=tile) as k:
        k.expect(want, ws_bytes=ws_bytes, M=M, N=N, K=K, epi=3)
        prob = _Problem(M, N, K, seed=M + N + K, w2=True)
        out, check = framed_out(M, N, 8, G)
        ws, check_ws = framed_ws(ws_bytes) if ws_bytes else (None, lambda: None)
        ops.gemm(prob.a, prob.w, w2=prob.w2, epi=3, out=out, ws=ws)
        _sync()
    r, c = _rows_cols_rel_l2(out, torch.nn.functional.silu(prob.core) * prob.core2, f"gate/up tile={tile} {shape}")
    check(); check_ws()
    print(f"gate/up tile={tile} {shape}: worst row {r:.2e}, worst column {c:.2e}")


# ---- W8A8 --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W8A8_SHAPES, ids=str)
def test_w8a8_elements(ops, shape):
    """vila_gemm_w8a8 on int8 operands drawn here (128 x 64 tile, K-tile 128; the kernel refuses K < 128, so K in {128, 144, 272}).  The int32
    accumulator is exact: bound = 2^-8 |ref| + 4 * 2^-24 * (|acc sx sw| + |bias| + |residual|), the 4 for one int-to-float conversion, two scale
    multiplies and the adds (gemm_i8.hip:148-169: fp32 throughout, rounded once).  int8 padding is 127, the scales' and bf16 operands' NaN."""
    from vila_amd import _lib
    lib = _lib.load()
    M, N, K = shape
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
    aq = framed_operand(torch.randint(-127, 128, (M, K), generator=g, device="cuda", dtype=torch.int8), 16, G, pad=127)
    wq = framed_operand(torch.randint(-127, 128, (N, K), generator=g, device="cuda", dtype=torch.int8), 16, G, pad=127)
    sx = framed_operand(torch.rand((M,), generator=g, device="cuda") * 0.02 + 0.005, 0, G)
    sw = framed_operand(torch.rand((N,), generator=g, device="cuda") * 0.002 + 0.0005, 0, G)
    bias, res = framed_operand(_rand((N,), 11), 0, G), framed_operand(_rand((M, N), 12), 4, G)
    acc = (aq.double() @ wq.double().t()) * sx.double()[:, None] * sw.double()[None, :]
    worst = 0.0
    for e in EPILOGUES:
        use_bias, use_res = "bias" in e, "residual" in e or e == "inplace"
        ref, mag = acc.clone(), acc.abs()
        if use_bias:
            ref += bias.double(); mag += bias.double().abs()
        if use_res:
            ref += res.double(); mag += res.double().abs()
        out, check = framed_out(M, N, 8, G, fill=res if e == "inplace" else None)
        r = out if e == "inplace" else res if use_res else None
        rc = lib.vila_gemm_w8a8(aq.data_ptr(), aq.stride(0), wq.data_ptr(), wq.stride(0), sx.data_ptr(), sw.data_ptr(), bias.data_ptr() if use_bias else None,
                                r.data_ptr() if r is not None else None, r.stride(0) if r is not None else 0, out.data_ptr(), out.stride(0), M, N, K, 0,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        _sync()
        worst = max(worst, assert_elementwise(out, ref, 2.0 ** -8 * ref.abs() + 4 * 2.0 ** -24 * mag, f"w8a8 {shape} [{e}]"))
        check()
    print(f"w8a8 {shape}: worst err / bound {worst:.3f}")


# ---- W4A16 prefill GEMM ----------------------------------------------------------------------------------------------------------------------------------
# gemm_w4.hip:9-11 / 148-165: per 128-wide group D = sum_k x_k (128 + q_k) on the matrix cores, s = sum_k x_k, acc += scale * (D - (128 + zero) * s).
# The magnitudes the kernel sums are therefore |x| . [scale (128 + q) + scale (128 + zero)], about 60 times |x| . |W_dequant|: the cancellation of the
# 128-offset is part of the kernel's error and of this bound (the accumulation term dominates it: the bound is valid, not sharp).  Three more fp32
# operations per group (subtract, multiply, fma) besides bias and residual.  Tile 64 rows x 128 packed rows, K % 128 == 0, N % 16 == 0; the entry
# point takes no leading dimensions, so x, residual and output are framed by guard rows only; the packed operands cannot carry NaN padding.
# Roundings as tests/test_gpu_w4_prefill.py::_check documents: one without a residual (gemm_w4.hip:64, 69); two with it, the projection + bias at
# ITS magnitude (gemm_w4.hip:68 bfround(v)) and the sum at the result's (gemm_w4.hip:69).  Under cancellation (projection ~ -residual) the first
# rounding is large against the result, so it is bounded by 2^-8 |projection + bias|, not folded into 2 * 2^-8 |result|, which no correct kernel meets.
def _w4_codes(mat):
    """logical arrays -> q [N, K], scale [N, G], 128 + zero [N, G] in fp64, natural row order."""
    wq, wsz = mat.logical
    N, K8 = wq.shape
    q = torch.empty((N, K8, 8), dtype=torch.float64, device=wq.device)
    for p in range(4):
        q[..., 2 * p] = ((wq >> (4 * p)) & 0xF).double()
        q[..., 2 * p + 1] = ((wq >> (4 * (p + 4))) & 0xF).double()
    scale = (wsz & 0xFFFF).to(torch.int16).view(torch.bfloat16).double()
    zp = ((wsz >> 16) & 0xFFFF).to(torch.int16).view(torch.bfloat16).double()
    return q.view(N, K8 * 8), scale, zp


def _w4_ref(x, mat):
    """-> fp64 x . W^T and the magnitudes the kernel sums, [M, rows of the logical matrix]."""
    q, scale, zp = _w4_codes(mat)
    K = q.shape[1]
    sc, z = scale.repeat_interleave(128, 1), zp.repeat_interleave(128, 1)
    assert sc.shape == (q.shape[0], K)
    xd = x.double()
    return xd @ ((q + 128.0 - z) * sc).t(), xd.abs() @ ((q + 128.0 + z) * sc).t()


def _w4_launch(lib, x, mat, bias, residual, out, mode, heads=None):
    M, K = x.shape
    nb = lib.vila_gemm_w4_workspace_bytes(M, mat.N, K, mode)
    ws, check_ws = framed_ws(nb) if nb else (None, lambda: None)
    p = lambda t: None if t is None else t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    if heads is not None:
        rc = lib.vila_gemm_w4_qkv_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), p(bias), out.data_ptr(), M, *heads, K, p(ws), nb, s)
    else:
        rc = lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), p(bias), p(residual), out.data_ptr(), M, mat.N, K, mode, p(ws), nb, s)
    assert rc == 0, lib.vila_last_error().decode()
    _sync()
    return nb, check_ws


W4_SHAPES = _grid((1, 63, 65, 144), (16, 112, 144), (128, 384, 640)) + [(65, 144, 4352)]


@pytest.mark.parametrize("shape", W4_SHAPES, ids=str)
def test_w4_plain_elements(ops, shape):
    """vila_gemm_w4_bf16 mode 0 with the 128-offset codes of test_gemm_w4_large_offsets_cancel in half the rows (q = 15, zero = 0) and seeded weights
    in the rest, activations with a mean; K = 128 runs unsliced (one group), the longer ones K-sliced with a workspace of exactly the bytes asked."""
    from vila_amd import _lib
    from vila_amd.quant import W4Matrix
    lib = _lib.load()
    M, N, K = shape
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    w = torch.randn((N, K), generator=g, device="cuda") * 0.02
    w[::2] = (15.0 * torch.exp2(-torch.randint(6, 10, (N, 1), generator=g, device="cuda").float())).expand(N, K)[::2]
    mat = W4Matrix.pack(w)
    x = framed_operand(((1.0 + torch.randn((M, K), generator=g, device="cuda"))).to(torch.bfloat16), 0, G)
    bias = framed_operand((torch.randn((N,), generator=g, device="cuda") * 0.5).to(torch.bfloat16), 0, G)
    res = framed_operand(_rand((M, N), 77), 0, G)
    core, core_abs = _w4_ref(x, mat)
    extra = 3 * (K // 128) + 2
    worst, slices = 0.0, set()
    for e in EPILOGUES:
        use_bias, use_res = "bias" in e, "residual" in e or e == "inplace"
        proj = core + bias.double() if use_bias else core.clone()
        absprod = core_abs + bias.double().abs() if use_bias else core_abs.clone()
        ref = proj + res.double() if use_res else proj
        bound = gemm_elem_bound(ref, absprod + (res.double().abs() if use_res else 0), K, roundings=1, extra_fp32_ops=extra)
        if use_res:
            bound = bound + gemm_elem_bound(proj, torch.zeros_like(proj), K, roundings=1)          # the second rounding, at the projection's magnitude
        out, check = framed_out(M, N, 0, G, fill=res if e == "inplace" else None)
        nb, check_ws = _w4_launch(lib, x, mat, bias if use_bias else None, out if e == "inplace" else res if use_res else None, out, 0)
        slices.add(nb)
        worst = max(worst, assert_elementwise(out, ref, bound, f"w4 {shape} [{e}]"))
        check(); check_ws()
    assert (K == 128) == (slices == {0}), f"K = {K}: workspace bytes {slices} (one group runs unsliced, more are K-sliced at these sizes)"
    print(f"w4 {shape}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("heads", [(2, 1, 16), (6, 2, 80)], ids=str)
def test_w4_qkv_elements(ops, M, heads):
    """vila_gemm_w4_qkv_bf16: q and k heads RoPE-interleaved in the packed matrix, written back in natural column order with the bias (one rounding)."""
    from vila_amd import _lib
    from vila_amd.quant import W4Matrix, rope_interleave_rows
    lib = _lib.load()
    nq, nkv, hd = heads
    N, K = (nq + 2 * nkv) * hd, 384
    g = torch.Generator(device="cuda").manual_seed(M + N)
    mat = W4Matrix.pack(torch.randn((N, K), generator=g, device="cuda") * 0.02, row_perm=rope_interleave_rows(nq + nkv, nq + 2 * nkv, hd, device="cuda"))
    x = framed_operand(torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16), 0, G)
    bias = framed_operand((torch.randn((N,), generator=g, device="cuda") * 0.5).to(torch.bfloat16), 0, G)
    core, core_abs = _w4_ref(x, mat)
    ref = core + bias.double()
    out, check = framed_out(M, N, 0, G)
    _, check_ws = _w4_launch(lib, x, mat, bias, None, out, 2, heads=heads)
    worst = assert_elementwise(out, ref, gemm_elem_bound(ref, core_abs + bias.double().abs(), K, extra_fp32_ops=3 * (K // 128) + 1), f"w4 qkv {heads} M={M}")
    check(); check_ws()
    print(f"w4 qkv {heads} M={M}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("M,N,K", [(65, 16, 128), (144, 80, 384)])
def test_w4_gateup_finite_and_framed(ops, M, N, K):
    """Mode 1 rounds gate, up and silu(gate) to bf16 before the product (gemm_w4.hip:55), so it keeps its whole-matrix tolerance (rel-L2 < 5e-3, as
    tests/test_gpu_w4_prefill.py); new here: every element finite, the output's guard rows and the workspace's guards intact."""
    from vila_amd import _lib
    from vila_amd.quant import W4Matrix
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    mat = W4Matrix.pack(torch.randn((N, K), generator=g, device="cuda") * 0.02, torch.randn((N, K), generator=g, device="cuda") * 0.02)
    x = framed_operand(torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16), 0, G)
    wg, wu = mat.dequantized()
    ref = torch.nn.functional.silu(x.double() @ wg.double().t()) * (x.double() @ wu.double().t())
    out, check = framed_out(M, N, 0, G)
    _, check_ws = _w4_launch(lib, x, mat, None, None, out, 1)
    assert bool(torch.isfinite(out).all())
    rel = float((out.double() - ref).norm() / ref.norm())
    assert rel < 5e-3, f"rel-L2 {rel:.3e}"
    check(); check_ws()

"""Every element of the three LoRA operators (vila_amd/csrc/lora.hip: vila_lora_down_bf16, vila_lora_up_bf16, vila_lora_wgrad_bf16) against the
derived bound of tests/lora_ref.py, in framed buffers, through the C entry points (the style of tests/test_gpu_train_elements.py).

Every case draws bf16 inputs, computes the reference in fp64 on those same values, calls the entry point twice with the output in a patterned
frame (guard rows, NaN-filled padding columns, every output element pre-filled with a NaN pattern), the operands between NaN guard rows and the
workspace between guard bytes, checks every element with assert_elementwise against
    gemm_elem_bound(ref, absprod, K_contraction, roundings=1, extra_fp32_ops=3)        (absprod includes |Res| / the old G)
asserts frames and workspace guards intact and the two calls bit-equal, synchronises after each launch and ends the session on a device error.
The cases and the dispatch edge each one is for are listed in tests/lora_ref.py; tests/test_lora_cpu.py proves the bound at the same cases.

Measured on MI355X, worst err / bound over all cases (a bf16 output reaches 0.996 by its final rounding alone): down 0.996, up 0.996, wgrad 0.994.
No case exposed a kernel fault."""
import pytest
import torch

from tests import lora_ref as LR
from tests.gpu_util import assert_elementwise, framed_operand, framed_out, framed_ws

pytestmark = pytest.mark.gpu

G = 4                                                    # guard rows on each side of every framed operand and output


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib
    return _lib.load()


def _stream():
    from vila_amd.ops import _stream as s
    return s()


def _sync():
    """Wait for the launch; a fault of the device ends the session there, so that nothing more is launched on it."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU faulted, nothing more is launched: {e}", returncode=3)


def _ok(rc, what):
    from vila_amd import _lib
    _lib.check(rc, what)
    _sync()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ws(n_bytes):
    if n_bytes == 0:
        return None, 0, lambda: None
    ws, check = framed_ws(n_bytes)
    assert ws.data_ptr() % 16 == 0
    return ws.data_ptr(), n_bytes, check


WORST = {}


def _note(op, worst):
    WORST[op] = max(WORST.get(op, 0.0), worst)
    print(f"{op}: worst err / bound {worst:.3f} (so far {WORST[op]:.3f})")


def _ids(cases):
    return ["-".join(str(int(v)) for v in c) for c in cases]


# ---- down ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(enumerate(LR.DOWN_CASES)), ids=_ids(LR.DOWN_CASES))
def test_lora_down_elements(lib, case):
    i, (M, K, R, pad) = case
    scale = LR.case_scale(i)
    x, a = (t.cuda() for t in LR.down_inputs(M, K, R))
    xf, af = framed_operand(x, 8, G), framed_operand(a, 16, G)
    ref, bound = LR.down_ref(x, a, scale)
    n_ws = int(lib.vila_lora_down_workspace_bytes(M, K, R))
    assert (n_ws > 0) == (LR.down_split(M, K)[0] > 1) and n_ws == (LR.down_split(M, K)[0] * M * R * 4 if n_ws else 0)
    outs = []
    for _ in range(2):
        out, check = framed_out(M, R, pad, G)
        ws, n, check_ws = _ws(n_ws)
        _ok(lib.vila_lora_down_bf16(xf.data_ptr(), xf.stride(0), af.data_ptr(), af.stride(0), out.data_ptr(), out.stride(0), M, K, R, scale, ws, n,
                                    _stream()), "lora_down")
        worst = assert_elementwise(out, ref, bound, f"lora_down [{M}, {K}] R={R}")
        check(); check_ws()
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"lora_down [{M}, {K}] R={R}: two calls differ"
    _note("lora_down", worst)


# ---- up -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(enumerate(LR.UP_CASES)), ids=_ids(LR.UP_CASES))
def test_lora_up_elements(lib, case):
    i, (M, N, R, with_res, pad) = case
    scale = LR.case_scale(i)
    t, bt, res = (v.cuda() for v in LR.up_inputs(M, N, R))
    tf, btf = framed_operand(t, 16 if i % 2 else 0, G), framed_operand(bt, 8, G)     # T as a column slice of a wider stack in every other case
    resf = framed_operand(res, pad + 8, G) if with_res else None
    ref, bound = LR.up_ref(t, bt, res if with_res else None, scale)
    assert int(lib.vila_lora_up_workspace_bytes(M, N, R)) == 0
    outs = []
    for _ in range(2):
        out, check = framed_out(M, N, pad, G)                                        # pad > 0: Y is a column slice
        _ok(lib.vila_lora_up_bf16(tf.data_ptr(), tf.stride(0), btf.data_ptr(), btf.stride(0), None if resf is None else resf.data_ptr(),
                                  0 if resf is None else resf.stride(0), out.data_ptr(), out.stride(0), M, N, R, scale, None, 0, _stream()), "lora_up")
        worst = assert_elementwise(out, ref, bound, f"lora_up [{M}, {N}] R={R} res={with_res}")
        check()
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"lora_up [{M}, {N}] R={R}: two calls differ"
    _note("lora_up", worst)


# ---- wgrad --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(enumerate(LR.WGRAD_CASES)), ids=_ids(LR.WGRAD_CASES))
def test_lora_wgrad_elements(lib, case):
    i, (M, C, R, accumulate, pad) = case
    scale = LR.case_scale(i)
    l, x, old = (v.cuda() for v in LR.wgrad_inputs(M, C, R))
    lf, xf = framed_operand(l, pad, G), framed_operand(x, 8, G)                     # pad > 0: L is a column slice of a wider stack
    ref, bound = LR.wgrad_ref(l, x, old if accumulate else None, scale)
    n_ws = int(lib.vila_lora_wgrad_workspace_bytes(M, R, C))
    assert (n_ws > 0) == (LR.wgrad_split(M, C)[0] > 1) and n_ws == (LR.wgrad_split(M, C)[0] * R * C * 4 if n_ws else 0)
    outs = []
    for _ in range(2):
        out, check = framed_out(R, C, 8, G, fill=old if accumulate else None)
        ws, n, check_ws = _ws(n_ws)
        _ok(lib.vila_lora_wgrad_bf16(lf.data_ptr(), lf.stride(0), xf.data_ptr(), xf.stride(0), out.data_ptr(), out.stride(0), M, R, C, scale,
                                     int(accumulate), ws, n, _stream()), "lora_wgrad")
        worst = assert_elementwise(out, ref, bound, f"lora_wgrad [{M}, {C}] R={R} acc={accumulate}")
        check(); check_ws()
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"lora_wgrad [{M}, {C}] R={R}: two calls differ"
    _note("lora_wgrad", worst)


# ---- constraint violations ----------------------------------------------------------------------------------------------------------------------
def test_constraint_violations_launch_nothing(lib):
    """A misaligned leading dimension or base pointer, an R that is no multiple of 16 (or above 192), a K / N / C that is no multiple of 8 and a
    workspace that is too small each return the library's error code and leave the framed output untouched."""
    M, K, R, N = 40, 1024, 32, 72
    x, a = (t.cuda() for t in LR.down_inputs(M, K, R))
    t, bt, res = (v.cuda() for v in LR.up_inputs(M, N, R))
    big = torch.zeros((64, 1024), dtype=torch.bfloat16, device="cuda")
    n_ws = int(lib.vila_lora_down_workspace_bytes(M, K, R))
    ws = torch.empty((n_ws,), dtype=torch.uint8, device="cuda")
    S = _stream()

    def untouched(rc, out, check, what):
        _sync()
        assert rc == -1, f"{what}: returned {rc}, expected the argument error -1"
        assert lib.vila_last_error(), what
        assert bool(torch.isnan(out).all()), f"{what}: the output was written"
        check()

    down = lambda xx, ldx, aa, lda, oo, ldo, m, k, r, w, n: lib.vila_lora_down_bf16(xx, ldx, aa, lda, oo, ldo, m, k, r, 1.0, w, n, S)
    for what, call in (
            ("down ldt % 8", lambda o: down(x.data_ptr(), K, a.data_ptr(), K, o.data_ptr(), R + 4, M, K, R, ws.data_ptr(), n_ws)),
            ("down ldx % 8", lambda o: down(x.data_ptr(), K + 4, a.data_ptr(), K, o.data_ptr(), o.stride(0), M, K, R, ws.data_ptr(), n_ws)),
            ("down R = 24", lambda o: down(x.data_ptr(), K, a.data_ptr(), K, o.data_ptr(), o.stride(0), M, K, 24, ws.data_ptr(), n_ws)),
            ("down R = 208", lambda o: down(big.data_ptr(), 1024, big.data_ptr(), 1024, o.data_ptr(), o.stride(0), M, K, 208, ws.data_ptr(), n_ws)),
            ("down K % 8", lambda o: down(x.data_ptr(), K, a.data_ptr(), K, o.data_ptr(), o.stride(0), M, K - 4, R, ws.data_ptr(), n_ws)),
            ("down X + 8 bytes", lambda o: down(x.data_ptr() + 8, K, a.data_ptr(), K, o.data_ptr(), o.stride(0), M - 1, K, R, ws.data_ptr(), n_ws)),
            ("down workspace too small", lambda o: down(x.data_ptr(), K, a.data_ptr(), K, o.data_ptr(), o.stride(0), M, K, R, ws.data_ptr(), n_ws - 16)),
            ("down no workspace", lambda o: down(x.data_ptr(), K, a.data_ptr(), K, o.data_ptr(), o.stride(0), M, K, R, None, 0))):
        out, check = framed_out(M, 208, 0, G)
        untouched(call(out), out, check, what)
    up = lambda tt, ldt, bb, ldb, rr, ldr, oo, ldo, m, n, r: lib.vila_lora_up_bf16(tt, ldt, bb, ldb, rr, ldr, oo, ldo, m, n, r, 1.0, None, 0, S)
    for what, call in (
            ("up ldy % 8", lambda o: up(t.data_ptr(), R, bt.data_ptr(), N, None, 0, o.data_ptr(), N + 4, M, N, R)),
            ("up ldres % 8", lambda o: up(t.data_ptr(), R, bt.data_ptr(), N, res.data_ptr(), N + 4, o.data_ptr(), o.stride(0), M, N, R)),
            ("up R = 40", lambda o: up(big.data_ptr(), 1024, bt.data_ptr(), N, None, 0, o.data_ptr(), o.stride(0), M, N, 40)),
            ("up N % 8", lambda o: up(t.data_ptr(), R, bt.data_ptr(), N, None, 0, o.data_ptr(), o.stride(0), M, N - 4, R)),
            ("up Res + 8 bytes", lambda o: up(t.data_ptr(), R, bt.data_ptr(), N, res.data_ptr() + 8, N, o.data_ptr(), o.stride(0), M - 1, N, R))):
        out, check = framed_out(M, N, 8, G)
        untouched(call(out), out, check, what)
    wg = lambda ll, ldl, xx, ldx, oo, ldo, m, r, c, w, n: lib.vila_lora_wgrad_bf16(ll, ldl, xx, ldx, oo, ldo, m, r, c, 1.0, 0, w, n, S)
    Mw = 300
    l, xw, _ = (v.cuda() for v in LR.wgrad_inputs(Mw, N, R))
    n_wg = int(lib.vila_lora_wgrad_workspace_bytes(Mw, R, N))
    assert n_wg > 0
    wsw = torch.empty((n_wg,), dtype=torch.uint8, device="cuda")
    for what, call in (
            ("wgrad ldg % 8", lambda o: wg(l.data_ptr(), R, xw.data_ptr(), N, o.data_ptr(), N + 4, Mw, R, N, wsw.data_ptr(), n_wg)),
            ("wgrad ldl % 8", lambda o: wg(l.data_ptr(), R + 4, xw.data_ptr(), N, o.data_ptr(), o.stride(0), Mw, R, N, wsw.data_ptr(), n_wg)),
            ("wgrad R = 8", lambda o: wg(l.data_ptr(), R, xw.data_ptr(), N, o.data_ptr(), o.stride(0), Mw, 8, N, wsw.data_ptr(), n_wg)),
            ("wgrad C % 8", lambda o: wg(l.data_ptr(), R, xw.data_ptr(), N, o.data_ptr(), o.stride(0), Mw, R, N - 4, wsw.data_ptr(), n_wg)),
            ("wgrad workspace too small", lambda o: wg(l.data_ptr(), R, xw.data_ptr(), N, o.data_ptr(), o.stride(0), Mw, R, N, wsw.data_ptr(), n_wg - 16))):
        out, check = framed_out(R, N, 8, G)
        untouched(call(out), out, check, what)


def test_ops_wrappers_match_the_entry_points(lib):
    """ops.lora_down / lora_up / lora_wgrad (their own workspace, column-sliced outputs) give the bits of the direct calls."""
    from vila_amd import ops
    M, K, R, N = 300, 1024, 32, 72
    x, a = (t.cuda() for t in LR.down_inputs(M, K, R))
    ref, bound = LR.down_ref(x, a, 0.5)
    stack = torch.full((M, 3 * R), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.lora_down(x, a, 0.5, out=stack[:, R:2 * R])
    _sync()
    assert_elementwise(stack[:, R:2 * R], ref, bound, "ops.lora_down into a stack's slice")
    assert bool(torch.isnan(stack[:, :R]).all()) and bool(torch.isnan(stack[:, 2 * R:]).all())
    t, bt, res = (v.cuda() for v in LR.up_inputs(M, N, R))
    ref, bound = LR.up_ref(t, bt, res, 2.0)
    assert_elementwise(ops.lora_up(t, bt, 2.0, res=res), ref, bound, "ops.lora_up")
    l, xw, old = (v.cuda() for v in LR.wgrad_inputs(M, N, R))
    ref, bound = LR.wgrad_ref(l, xw, old, 0.5)
    g = old.clone()
    assert_elementwise(ops.lora_wgrad(l, xw, g, 0.5, accumulate=True), ref, bound, "ops.lora_wgrad accumulate")
    _sync()
    with pytest.raises(ValueError):
        ops.lora_down(x, a[:24], 1.0)

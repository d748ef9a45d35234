"""Every element of the SFT operators (vila_amd/csrc/train.hip) and of the norm kernels (elementwise.hip) against a derived bound, in framed buffers.

The other tests of these operators judge a tensor by one rel-L2 number at one or a few shapes: a fault confined to one row tail, one column chunk,
one launch seam or one ignored label fits inside it (tests/test_train_bound_cpu.py shows which ones).  Here every case
  - draws bf16 inputs and computes the reference in fp64 on those same values;
  - calls the C entry point directly, with outputs in patterned frames (guard rows / guard elements, every element of the output pre-filled with
    a NaN pattern, so an element never written fails as non-finite) and inputs between NaN guard rows;
  - checks every output element with assert_elementwise against the bound of tests/gpu_util.py (each constant there cites the kernel lines it
    counts), or bit for bit where the kernel's arithmetic is exactly reproducible (scatter_add_rows, depth_to_space, bf16(master));
  - synchronises after each launch and ends the session on a device error.

Shapes: the smallest that straddle each dispatch edge -- the norm forward's 1536 / 4096 / 8192 columns, the backward's wave kernels (MAXI 7, 8, 3),
4096-column chunks and row blocks of 12 and 8, cross entropy's 256-thread stride and the step's 256-row chunk, the 8192-block grid cap of the
element-wise kernels, AdamW's pairs and its 2^28-pair launch seam.

Measured on MI355X, worst err / bound per operator over all of its cases (a bf16 output reaches 1 / (1 + 2^-8) = 0.996 by its final rounding alone):
    LayerNorm forward 0.995 (without b 0.994), RMSNorm forward 0.988; the two forms of the block kernel bit-equal at every width;
    norm backward, RMSNorm dx 0.995, dw 0.996; LayerNorm dx 0.995, dw 0.994, db 0.996; repeated calls bit-equal;
    cross entropy dlogits 0.995, loss 0.050; ignored rows exactly zero;
    GELU forward tanh 0.987, erf 0.975; backward 0.996 both; SwiGLU forward 0.988 (near-tie elements 0.8 % of the sweep), backward dg 0.996, du 0.996;
    AdamW master / m / v 0.558, at the launch seam 0.580, lean and plain bit-equal over all 2^29 + 11 elements;
    scatter_add_rows and depth_to_space: bit-exact.
No case exposed a kernel fault."""
import pytest
import torch

from tests.gpu_util import (adamw_bounds, assert_elementwise, ce_bounds, depth_to_space_index_map, framed_flat, framed_operand,
                            framed_out, gelu_erf_bwd_bound, gelu_erf_fwd_bound, gelu_tanh_bwd_bound, gelu_tanh_fwd_bound, layernorm_fwd_bound,
                            norm_bwd_bounds, norm_bwd_route, rmsnorm_fwd_bound, scatter_add_rows_ref, silu_mul_bwd_bound, silu_mul_fwd_bound)

pytestmark = pytest.mark.gpu

G = 4                                                    # guard rows on each side of every framed operand and output
EPS = 1e-6

# ---- the cases (tests/test_train_bound_cpu.py proves the bounds at these same shapes and inputs) ------------------------------------------------
NORM_FWD_COLS = [8, 1152, 1528, 1536, 1544, 3584, 4096, 4104, 4608, 8192, 8200, 13824, 16384]
NORM_FWD_ROWS = [1, 5, 7]                                # the wave kernel packs four rows per block
NORM_DISTS = ["wide", "offset"]                          # N(0, 2^2) + 0.5; mean 30, std 1 (punishes a one-pass variance)
NORM_BWD_CASES = ([(True, c, "aligned") for c in (8, 3584, 3592, 4096, 4104, 8200)] + [(False, c, "aligned") for c in (8, 1536, 1544, 4608, 13824)]
                  + [(rms, c, "aligned") for rms in (True, False) for c in (100, 4100)]             # cols % 8 != 0: the generic kernel
                  + [(True, 3584, "x+8B"), (False, 1152, "x+8B")])                                   # x only 8-byte aligned: the generic kernel
NORM_BWD_ROWS = [1, 8, 9, 11, 12, 13, 25, 60]            # row blocks of 12 (wave) and 8 (generic); 1-5 partials of the four-group reduce
CE_V = [8, 255, 256, 257, 1000, 152064]
CE_ROWS = [1, 5, 256, 600]                               # 256: the step's LOGIT_CHUNK; 600: the ordered sum's third pass
CE_KINDS = ["x3", "spread", "equal"]
SCATTER_N = [1, 50, 600]
SCATTER_H = [2, 512, 514, 3584]
SCATTER_PATTERNS = ["distinct", "equal", "mixed", "ends"]
D2S_GK = [(4, 2), (5, 2), (7, 2), (27, 2), (32, 2), (4, 3), (5, 3), (7, 3), (32, 3)]
ACT_BIG_N = 8 * (8192 * 256 + 5)                         # one 16-byte chunk per thread of the capped 8192-block grid, and five chunks more
ADAMW_N = [1, 2, 3, 5, 4123]
ADAMW_STEPS = [1, 2, 1000]
ADAMW_SEAM_N = (1 << 29) + 11                            # two lean launches (2^28 pairs each side of the seam) and the odd tail
ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bf(t, device):
    return t.to(torch.bfloat16).to(device)


def norm_inputs(rows, cols, dist, seed=0, device="cuda"):
    """-> x, w, b, dy (bf16)."""
    g = _gen(1000 * seed + rows + 7 * cols + (0 if dist == "wide" else 1))
    x = torch.randn(rows, cols, generator=g) * 2.0 + 0.5 if dist == "wide" else torch.randn(rows, cols, generator=g) + 30.0
    w = torch.randn(cols, generator=g) * 0.5 + 1.0
    b = torch.randn(cols, generator=g) * 0.5
    dy = torch.randn(rows, cols, generator=g)
    return _bf(x, device), _bf(w, device), _bf(b, device), _bf(dy, device)


def ce_inputs(rows, V, kind, device="cuda"):
    """-> logits [rows, V] fp32, labels [rows] int64.  Labels cycle through 0, V - 1, ignored, the arg-max (its logit raised so that p ~ 1) and a
    random class."""
    g = _gen(rows + 3 * V + CE_KINDS.index(kind))
    if kind == "x3":
        z = torch.randn(rows, V, generator=g) * 3.0
    elif kind == "spread":
        z = (torch.rand(rows, V, generator=g) * 2.0 - 1.0) * 40.0
    else:
        z = torch.full((rows, V), 7.25)
    lab = torch.randint(0, V, (rows,), generator=g)
    r = torch.arange(rows) + CE_KINDS.index(kind)
    lab[r % 5 == 0], lab[r % 5 == 1], lab[r % 5 == 2] = 0, V - 1, -100
    am = (r % 5 == 3).nonzero().flatten()
    if kind != "equal" and am.numel():
        top = z[am].argmax(-1)
        z[am, top] += 30.0
        lab[am] = top
    return z.to(device), lab.to(device)


def scatter_ids(n, T, pattern, seed=0):
    g = _gen(n + T + seed)
    if pattern == "distinct":
        ids = torch.randperm(T, generator=g)[:n]
    elif pattern == "equal":
        ids = torch.full((n,), T // 2)
    elif pattern == "mixed":
        ids = torch.randint(0, max(2, n // 4), (n,), generator=g)
    else:
        ids = torch.randint(0, T, (n,), generator=g)
        ids[0::3], ids[1::3] = 0, T - 1
    return ids.to(torch.int32)


def act_sweep(device="cuda"):
    """Every finite bf16 value with |z| <= 2^16, both signs, padded with zeros to a multiple of 8."""
    bits = torch.arange(0, 0x7F80, dtype=torch.int32)
    bits = torch.cat([bits, bits + 0x8000]).to(torch.uint16).view(torch.bfloat16)
    z = bits[bits.float().abs() <= 65536.0]
    pad = (-z.numel()) % 8
    return torch.cat([z, torch.zeros(pad, dtype=torch.bfloat16)]).to(device)


def act_inputs(kind, device="cuda"):
    """-> z (or g), dy (or u), da."""
    z = act_sweep(device) if kind == "sweep" else _bf(torch.randn(ACT_BIG_N, generator=_gen(5)) * 2.0, device)
    g = _gen(6 + z.numel() % 97)
    return z, _bf(torch.randn(z.numel(), generator=g), device), _bf(torch.randn(z.numel(), generator=g), device)


def adamw_state(n, seed=0, device="cuda"):
    """-> master, m, v (fp32), grad (bf16): random non-zero m, v >= 0, and (n >= 5) a block of zero gradients with zero state."""
    g = _gen(n + seed)
    p, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v, gr = torch.rand(n, generator=g) * 0.01 + 1e-6, torch.randn(n, generator=g)
    if n >= 5:
        z = slice(1, 3) if n < 200 else slice(100, 164)
        m[z], v[z], gr[z] = 0.0, 0.0, 0.0
    return p.to(device), m.to(device), v.to(device), _bf(gr, device)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib
    return _lib.load()


def _stream():
    from vila_amd.ops import _stream as s
    return s()


def _ok(rc, what):
    from vila_amd import _lib
    _lib.check(rc, what)
    _sync()


def _sync():
    """Wait for the launch; a fault of the device ends the session there, so that nothing more is launched on it."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU faulted, nothing more is launched: {e}", returncode=3)


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


WORST = {}


def _note(op, worst):
    WORST[op] = max(WORST.get(op, 0.0), worst)
    print(f"{op}: worst err / bound {worst:.3f} (so far {WORST[op]:.3f})")


# ---- 1. LayerNorm / RMSNorm forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ln", "ln_nob", "rms"])
@pytest.mark.parametrize("cols", NORM_FWD_COLS)
def test_norm_forward_elements(lib, cols, kind):
    """All three kernels (norm_wave_kernel up to 1536 columns, the block kernel in its up-front-load form and its plain form above), rows 1 / 5 / 7,
    two input distributions.  The two forms of the block kernel must agree bit for bit."""
    worst = 0.0
    try:
        for rows in NORM_FWD_ROWS:
            for dist in NORM_DISTS:
                x, w, b, _ = norm_inputs(rows, cols, dist)
                xf, wf, bf = framed_operand(x, 0, G), framed_operand(w, 0, G), (framed_operand(b, 0, G) if kind == "ln" else None)
                if kind == "rms":
                    ref, bound, _, _ = rmsnorm_fwd_bound(x.double(), w.double(), EPS)
                else:
                    ref, bound, _ = layernorm_fwd_bound(x.double(), w.double(), None if bf is None else b.double(), EPS)
                outs = []
                for lat in ((1, 0) if cols > 1536 else (-1,)):
                    lib.vila_norm_force_lat(lat)
                    out, check = framed_out(rows, cols, 0, G)
                    if kind == "rms":
                        _ok(lib.vila_rmsnorm_bf16(xf.data_ptr(), wf.data_ptr(), out.data_ptr(), rows, cols, EPS, _stream()), "rmsnorm")
                    else:
                        _ok(lib.vila_layernorm_bf16(xf.data_ptr(), wf.data_ptr(), _p(bf), out.data_ptr(), rows, cols, EPS, _stream()), "layernorm")
                    worst = max(worst, assert_elementwise(out, ref, bound, f"{kind} [{rows}, {cols}] {dist} lat={lat}"))
                    check()
                    outs.append(out)
                if len(outs) == 2:
                    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{kind} [{rows}, {cols}] {dist}: the up-front-load form differs from the plain form"
    finally:
        lib.vila_norm_force_lat(-1)
    _note("norm_fwd " + kind, worst)


# ---- 2. norm backward -------------------------------------------------------------------------------------------------------------------------------
def _norm_bwd_call(lib, x, w, dy, dx, dw, db, rows, cols, rms, accumulate):
    n = int(lib.vila_norm_bwd_scratch_floats(rows, cols))
    scratch, check = framed_flat(n, torch.float32)
    _ok(lib.vila_norm_bwd_bf16(x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), _p(db), scratch.data_ptr(), rows, cols, EPS,
                               int(rms), int(accumulate), _stream()), "norm_bwd")
    check()


@pytest.mark.parametrize("rms,cols,align", NORM_BWD_CASES, ids=lambda v: str(v))
def test_norm_backward_elements(lib, rms, cols, align):
    """dx, dw, db of the wave kernels and of the generic kernel (wide rows, cols % 8 != 0, an x pointer that is only 8-byte aligned), every row count
    of NORM_BWD_ROWS, accumulate off and on with preset dw / db, LayerNorm without db, and two calls bit-identical."""
    worst = {"dx": 0.0, "dw": 0.0, "db": 0.0}
    for rows in NORM_BWD_ROWS:
        x, w, _, dy = norm_inputs(rows, cols, "wide", seed=1)
        if align == "x+8B":
            buf = torch.full((rows * cols + 64,), float("nan"), dtype=torch.bfloat16, device="cuda")
            xf = buf[20:20 + rows * cols].view(rows, cols)
            xf.copy_(x)
            assert xf.data_ptr() % 16 == 8
        else:
            xf = framed_operand(x, 0, G)
        wf, dyf = framed_operand(w, 0, G), framed_operand(dy, 0, G)
        route = norm_bwd_route(rows, cols, rms, aligned=(align == "aligned"))
        old_w = (torch.randn(cols, generator=_gen(rows + cols)) * 2.0).to(torch.bfloat16).cuda()
        old_b = (torch.randn(cols, generator=_gen(rows + cols + 1)) * 2.0).to(torch.bfloat16).cuda()
        for accumulate, with_db in ((False, True), (True, True), (False, False)):
            if rms and not with_db:
                continue
            want = norm_bwd_bounds(x.double(), w.double(), dy.double(), EPS, rms, route, old_w.double() if accumulate else None,
                                   old_b.double() if accumulate else None)
            got = []
            for _ in range(2):
                dx, check_dx = framed_out(rows, cols, 0, G)
                dw, check_dw = framed_out(1, cols, 8, G, fill=old_w[None] if accumulate else None)
                db, check_db = framed_out(1, cols, 8, G, fill=old_b[None] if accumulate else None)
                use_db = (not rms) and with_db
                _norm_bwd_call(lib, xf, wf, dyf, dx, dw, db if use_db else None, rows, cols, rms, accumulate)
                what = f"{'rms' if rms else 'ln'} bwd [{rows}, {cols}] {align} acc={accumulate} db={use_db}"
                worst["dx"] = max(worst["dx"], assert_elementwise(dx, want["dx"][0], want["dx"][1], what + " dx"))
                worst["dw"] = max(worst["dw"], assert_elementwise(dw, want["dw"][0][None], want["dw"][1][None], what + " dw"))
                if use_db:
                    worst["db"] = max(worst["db"], assert_elementwise(db, want["db"][0][None], want["db"][1][None], what + " db"))
                elif not accumulate:
                    assert bool(torch.isnan(db).all()), what + ": db written although none was passed"
                check_dx(); check_dw(); check_db()
                got.append((dx, dw, db))
            for a, b in zip(*got):
                assert torch.equal(_bits(a), _bits(b)), what + ": two calls differ"
    for k, v in worst.items():
        _note(f"norm_bwd {'rms' if rms else 'ln'} {k}", v)


# ---- 3. cross entropy -------------------------------------------------------------------------------------------------------------------------------
def _ce_call(lib, z, lab, rows, V, scale, loss0):
    zf = framed_operand(z, 24, G)                                         # ldl = V + 24, NaN padding
    d, check_d = framed_flat(rows * V)
    loss, check_loss = framed_flat(1, torch.float32, fill=torch.tensor([loss0]))
    row_loss, check_rl = framed_flat(rows, torch.float32)
    _ok(lib.vila_ce_loss_f32(zf.data_ptr(), lab.data_ptr(), d.data_ptr(), loss.data_ptr(), row_loss.data_ptr(), rows, V, zf.stride(0), scale, _stream()),
        "ce_loss")
    check_d(); check_loss(); check_rl()
    return d.view(rows, V), loss


@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_elements(lib, V):
    """Every dlogits element and the scalar loss: V around the 256-thread stride and the model's 152 064, rows 1 / 5 / 256 / 600, ldl = V + 24, labels
    0, V - 1, ignored (-100: the gradient row is exactly zero and adds exactly 0 to the loss), the arg-max with p ~ 1; logits * 3, a +-40 spread,
    all equal; scale != 1 and the loss accumulator preloaded with 1.5."""
    worst_d = worst_l = 0.0
    scale, loss0 = 1.0 / 29.0, 1.5
    for rows in ([3] if V == 152064 else CE_ROWS):
        for kind in CE_KINDS:
            z, lab = ce_inputs(rows, V, kind)
            d, loss = _ce_call(lib, z, lab, rows, V, scale, loss0)
            dref, dbound, _, loss_ref, loss_bound = ce_bounds(z.double(), lab, scale, loss0)
            what = f"ce [{rows}, {V}] {kind}"
            worst_d = max(worst_d, assert_elementwise(d, dref, dbound, what))
            ign = lab == -100
            assert bool((_bits(d)[ign] == 0).all()), what + ": an ignored row's gradient is not exactly zero"
            err = abs(float(loss) - loss_ref)
            print(f"{what}: loss {float(loss):.7f} ref {loss_ref:.7f} err / bound {err / loss_bound:.3f}")
            assert err <= loss_bound, f"{what}: loss {float(loss)} vs fp64 {loss_ref} (err {err:.3e}, bound {loss_bound:.3e})"
            worst_l = max(worst_l, err / loss_bound)
    z, _ = ce_inputs(5, V, "x3")
    d, loss = _ce_call(lib, z, torch.full((5,), -100, dtype=torch.int64, device="cuda"), 5, V, scale, loss0)
    assert bool((_bits(d) == 0).all()) and float(loss) == loss0, f"ce V={V}: ignored rows must leave zeros and the loss untouched (loss {float(loss)})"
    _note("ce dlogits", worst_d)
    _note("ce loss", worst_l)


# ---- 4. scatter_add_rows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", SCATTER_H)
@pytest.mark.parametrize("n", SCATTER_N)
def test_scatter_add_rows_is_the_documented_sum(lib, n, H):
    """Bit-exact against the documented order (first occurrence, later ones ascending in fp32, old + sum rounded once) into a table of random bf16;
    untouched rows stay bit-identical, two calls agree bit for bit."""
    T = n + 3
    g = _gen(n + H)
    src = _bf(torch.randn(n, H, generator=g), "cuda")
    table = _bf(torch.randn(T, H, generator=g) * 2.0, "cuda")
    srcf = framed_operand(src, 0, G)
    for pattern in SCATTER_PATTERNS:
        ids = scatter_ids(n, T, pattern).cuda()
        ref = scatter_add_rows_ref(src, table, ids)
        got = []
        for _ in range(2):
            flat, check = framed_flat(T * H, fill=table)                 # (H = 2 and 514: rows that are only 4-byte aligned)
            dst = flat.view(T, H)
            _ok(lib.vila_scatter_add_rows_bf16(srcf.data_ptr(), dst.data_ptr(), ids.data_ptr(), n, H, _stream()), "scatter_add_rows")
            check()
            diff = (_bits(dst) != _bits(ref)).nonzero()
            assert diff.numel() == 0, f"scatter n={n} H={H} {pattern}: {diff.shape[0]} elements differ from the documented sum, first (row, col) {diff[0].tolist()}"
            got.append(dst)
        assert torch.equal(_bits(got[0]), _bits(got[1]))
        untouched = torch.ones(T, dtype=torch.bool, device="cuda")
        untouched[ids.long()] = False
        assert torch.equal(_bits(got[0])[untouched], _bits(table)[untouched]), f"scatter n={n} H={H} {pattern}: a row no id names changed"


# ---- 5. depth_to_space ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 1152])
@pytest.mark.parametrize("g,k", D2S_GK)
def test_depth_to_space_is_the_oracle_permutation(lib, g, k, C):
    """Bit-exact against the index map of the oracle's downsample_block; dx is framed and pattern-filled, so every element must be written."""
    for B in (1, 3):
        gd = (g + k - 1) // k
        dy = _bf(torch.randn(B * gd * gd, k * k * C, generator=_gen(g + k + C + B)), "cuda")
        dyf = framed_operand(dy, 0, G)
        dx, check = framed_flat(B * g * g * C)
        _ok(lib.vila_depth_to_space_bf16(dyf.data_ptr(), dx.data_ptr(), B, g, C, k, _stream()), "depth_to_space")
        check()
        pos = depth_to_space_index_map(B, g, k).cuda()
        ref = dy.view(-1, C)[pos.view(-1)]
        diff = (_bits(dx.view(-1, C)) != _bits(ref)).nonzero()
        assert diff.numel() == 0, f"depth_to_space B={B} g={g} k={k} C={C}: {diff.shape[0]} elements differ, first (cell, channel) {diff[0].tolist()}"


# ---- 6. activations and SwiGLU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sweep", "big"])
def test_activation_elements(lib, kind):
    """act_fwd / act_bwd (tanh and erf GELU), silu_mul and silu_mul_bwd over every finite bf16 z with |z| <= 2^16, and at n = 8 (8192 * 256 + 5), where
    the grid-stride loop takes a second pass."""
    z, dy, da = act_inputs(kind)
    n = z.numel()
    z64, dy64, da64 = z.double(), dy.double(), da.double()
    zf, dyf, daf = (framed_operand(t, 0, 1) for t in (z, dy, da))
    for act, fwd, bwd in ((1, gelu_tanh_fwd_bound, gelu_tanh_bwd_bound), (2, gelu_erf_fwd_bound, gelu_erf_bwd_bound)):
        y, check = framed_flat(n)
        _ok(lib.vila_act_fwd_bf16(zf.data_ptr(), y.data_ptr(), n, act, _stream()), "act_fwd")
        check()
        ref, bound, _ = fwd(z64)
        _note(f"act_fwd {act}", assert_elementwise(y[None], ref[None], bound[None], f"act_fwd act={act} {kind}"))
        dz, check = framed_flat(n)
        _ok(lib.vila_act_bwd_bf16(zf.data_ptr(), dyf.data_ptr(), dz.data_ptr(), n, act, _stream()), "act_bwd")
        check()
        ref, bound, _ = bwd(z64, dy64)
        _note(f"act_bwd {act}", assert_elementwise(dz[None], ref[None], bound[None], f"act_bwd act={act} {kind}"))
        del ref, bound
    a, check = framed_flat(n)
    _ok(lib.vila_silu_mul_fwd_bf16(zf.data_ptr(), dyf.data_ptr(), a.data_ptr(), n, _stream()), "silu_mul")
    check()
    ref, bound, _, near = silu_mul_fwd_bound(z64, dy64)
    assert float(near.double().mean()) < 0.01
    _note("silu_mul", assert_elementwise(a[None], ref[None], bound[None], f"silu_mul {kind}"))
    dg, check_g = framed_flat(n)
    du, check_u = framed_flat(n)
    _ok(lib.vila_silu_mul_bwd_bf16(zf.data_ptr(), dyf.data_ptr(), daf.data_ptr(), dg.data_ptr(), du.data_ptr(), n, _stream()), "silu_mul_bwd")
    check_g(); check_u()
    (rg, bg, _), (ru, bu, _) = silu_mul_bwd_bound(z64, dy64, da64)
    _note("silu_mul_bwd dg", assert_elementwise(dg[None], rg[None], bg[None], f"silu_mul_bwd dg {kind}"))
    _note("silu_mul_bwd du", assert_elementwise(du[None], ru[None], bu[None], f"silu_mul_bwd du {kind}"))


# ---- 7. AdamW ---------------------------------------------------------------------------------------------------------------------------------------
def _adamw_call(lib, lean, st, grad, param, n, wd, step, gs):
    fn = lib.vila_adamw_step_lean if lean else lib.vila_adamw_step
    hp = ADAMW_HP
    _ok(fn(st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), grad.data_ptr(), param.data_ptr(), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, step, gs,
           _stream()), "adamw")


@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_elements(lib, n):
    """Both kernels, element by element against an fp64 AdamW (bias corrections in fp64) from a random state: steps 1, 2, 1000, weight decay 0 and
    0.1, grad_scale 1 and 0.37; master, m and v each within their bound, param == bf16(master) bit for bit, the guards around every buffer intact."""
    p0, m0, v0, grad = adamw_state(n)
    gf, _ = framed_flat(n, fill=grad)
    worst = 0.0
    for step in ADAMW_STEPS:
        for wd in (0.0, 0.1):
            for gs in (1.0, 0.37):
                want = adamw_bounds(p0.double(), m0.double(), v0.double(), grad.double(), wd=wd, step=step, grad_scale=gs, **ADAMW_HP)
                for lean in (False, True):
                    frames = [framed_flat(n, torch.float32, fill=t) for t in (p0, m0, v0)]
                    param, check_param = framed_flat(n)
                    _adamw_call(lib, lean, [f[0] for f in frames], gf, param, n, wd, step, gs)
                    what = f"adamw{'_lean' if lean else ''} n={n} step={step} wd={wd} gs={gs}"
                    for (name, (ref, bound)), (buf, check) in zip(want.items(), frames):
                        worst = max(worst, assert_elementwise(buf[None], ref[None], bound[None], f"{what} {name}"))
                        check()
                    check_param()
                    assert torch.equal(_bits(param), _bits(frames[0][0].to(torch.bfloat16))), what + ": param != bf16(master)"
    _note("adamw", worst)


def test_adamw_launch_seam(lib):
    """n = 2^29 + 11: the lean kernel's two launches of 2^28 pairs, a five-pair third and the odd tail (the 8B embedding bucket crosses this seam in
    every step).  Lean and plain agree bit for bit over the whole buffer; both meet the fp64 bound in 4096-element windows at the start, around
    2^29 and at the end."""
    n = ADAMW_SEAM_N
    gen = torch.Generator(device="cuda").manual_seed(29)
    sets = [[framed_flat(n, torch.float32) for _ in range(3)] for _ in range(2)]
    grad, _ = framed_flat(n)
    step_ = 1 << 26
    for i in range(0, n, step_):
        k = min(step_, n - i)
        for j, (mul, add, sq) in enumerate(((1.0, 0.0, False), (0.1, 0.0, False), (0.01, 1e-6, True))):
            r = torch.randn(k, device="cuda", generator=gen)
            r = (r * r if sq else r) * mul + add
            sets[0][j][0][i:i + k] = r
            sets[1][j][0][i:i + k] = r
        grad[i:i + k] = torch.randn(k, device="cuda", generator=gen).to(torch.bfloat16)
    windows = [slice(0, 4096), slice((1 << 29) - 2048, (1 << 29) + 11), slice(n - 4096, n)]
    before = [[sets[0][j][0][w].clone() for j in range(3)] + [grad[w].clone()] for w in windows]
    params = [framed_flat(n) for _ in range(2)]
    wd, step, gs = 0.1, 3, 0.37
    for lean in (0, 1):
        _adamw_call(lib, bool(lean), [f[0] for f in sets[lean]], grad, params[lean][0], n, wd, step, gs)
        for _, check in sets[lean]:
            check()
        params[lean][1]()
    for j, name in enumerate(("master", "m", "v")):
        assert torch.equal(_bits(sets[0][j][0]), _bits(sets[1][j][0])), f"adamw seam: lean and plain differ in {name}"
    assert torch.equal(_bits(params[0][0]), _bits(params[1][0])), "adamw seam: lean and plain differ in param"
    worst = 0.0
    for w, (p0, m0, v0, g0) in zip(windows, before):
        want = adamw_bounds(p0.double(), m0.double(), v0.double(), g0.double(), wd=wd, step=step, grad_scale=gs, **ADAMW_HP)
        for j, (name, (ref, bound)) in enumerate(want.items()):
            worst = max(worst, assert_elementwise(sets[1][j][0][w][None], ref[None], bound[None], f"adamw seam window {w.start} {name}"))
        assert torch.equal(_bits(params[1][0][w]), _bits(sets[1][0][0][w].to(torch.bfloat16))), f"adamw seam window {w.start}: param != bf16(master)"
    _note("adamw seam", worst)

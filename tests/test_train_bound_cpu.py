"""The element-wise bounds of the SFT operators and the norms (tests/gpu_util.py), proved on the CPU before they judge a kernel
(tests/test_gpu_train_elements.py), at that file's shapes and inputs (element-wise operators at n = 8 (8192 * 256 + 5): the first and last 2^17
elements; the AdamW seam: random windows -- the bounds are per element).

  - Each bound admits an fp32 torch emulation of the kernel's formula in two summation orders (torch's own sum; 64 lanes that each add their
    strided elements, then a sum over the lanes): worst err / bound <= 1.  Observed worst over the cases of an operator, smallest - largest (both
    orders): LayerNorm forward 0.51 - 0.995, RMSNorm forward 0.64 - 0.988, backward dx 0.66 - 0.995, dw 0.45 - 0.995, db up to 0.996, cross
    entropy dlogits up to 0.995, GELU / SwiGLU forward and backward 0.965 - 0.996, AdamW master / m / v up to 0.54 / 0.50 / 0.56.  A bf16 output
    sits at up to 1 / (1 + 2^-8) = 0.996 of the bound by its final rounding alone (half a spacing against 2^-8 |ref| just above a power of two): what
    the bound leaves beyond a correct kernel is the accumulation term, which the sharpness check below keeps small.
  - The check stays sharp: the accumulation term is below the rounding term for at least 99 % of the elements of every case, with two derived
    exceptions stated at SHARP_EXCEPTIONS; RMSNorm's and SwiGLU's near-tie elements are under 1 % of every case.
  - The bound rejects each injected fault:
      one dw column summed without its last row block; the last row's dx formed with the previous row's statistics; LayerNorm without b on one
      8-column chunk; an ignored label's row not zeroed; a duplicate id added twice; AdamW's element 2 * n2 (the odd tail) skipped; the element at
      the 2^29 launch seam skipped.
  - The first three of those faults PASS the rel-L2 assertions of tests/test_gpu_train.py::test_norm_backward (< 1e-2) and
    tests/test_gpu_ops.py::test_layernorm_rmsnorm (< 3e-3) on those tests' own inputs, and FAIL the new check."""
import pytest
import torch

from tests.gpu_util import (BF16_U, FP32_U, adamw_bounds, assert_elementwise, ce_bounds, depth_to_space_index_map, framed_flat,
                            gelu_erf_bwd_bound, gelu_erf_fwd_bound, gelu_tanh_bwd_bound, gelu_tanh_fwd_bound, GELU_K0, GELU_K1, ERF_C, PDF_C,
                            layernorm_fwd_bound, norm_bwd_bounds, norm_bwd_route, randn_bf16, rel_l2, rmsnorm_fwd_bound, scatter_add_rows_ref,
                            silu_mul_bwd_bound, silu_mul_fwd_bound)
from tests.test_gpu_train_elements import (ACT_BIG_N, ADAMW_HP, ADAMW_N, ADAMW_SEAM_N, ADAMW_STEPS, CE_KINDS, CE_ROWS, CE_V, D2S_GK, EPS, NORM_BWD_CASES,
                                           NORM_BWD_ROWS, NORM_DISTS, NORM_FWD_COLS, NORM_FWD_ROWS, act_inputs, adamw_state,
                                           ce_inputs, norm_inputs, scatter_ids)

ORDERS = (0, 1)

# Where the accumulation term cannot stay below the rounding term for 99 % of the elements, and why; the fraction asserted instead.
#   "offset": the inputs with mean 30 and std 1.  The mean's own fp32 error, depth * 2^-24 * 30, is an absolute error of x - mean; it outweighs the
#       rounding 2^-8 |y| of every output with |y| < (depth + 8) * 2^-16 * 60 |w| (0.02 - 0.05 for y ~ N(0, 1)): 2 - 4 % of the elements in expectation,
#       and a case of 1152 elements spreads by another 1.7 % (3 sigma).  That cancellation is what the distribution is there to exercise.
#   "colsum": dw / db are sums over the rows that cancel (|sum| ~ sqrt(rows) against sum |.| ~ rows), so at 25 and 60 rows of the widest generic
#       rows (stat depth 63) up to 2 % of the columns have a sum below the absolute term.
SHARP_MIN = 0.99
MIN_COUNT = 1000            # fractions are asserted on cases of at least this many elements: one element of an 8-column case is already 2 - 12 %
SHARP_EXCEPTIONS = {"offset": 0.94, "colsum": 0.97}


def _sum32(t, dim, order):
    """fp32 sum along dim in one of two orders."""
    t = t.float().movedim(dim, -1)
    if order == 0:
        return t.sum(-1)
    pad = (-t.shape[-1]) % 64
    t = torch.cat([t, t.new_zeros(t.shape[:-1] + (pad,))], -1)
    return t.reshape(t.shape[:-1] + (-1, 64)).sum(-2).sum(-1)


def _sharp(ref, acc, roundings=1):
    return float(((1.0 + BF16_U) * FP32_U * acc <= roundings * BF16_U * ref.abs()).double().mean())


def _admit(out, ref, bound, what):
    w = assert_elementwise(out, ref, bound, what)
    assert w <= 1.0
    return w


# ---- fp32 emulations of the kernels' formulas ----------------------------------------------------------------------------------------------------
def _emu_stats(x, rms, order):
    cols = x.shape[-1]
    x32 = x.float()
    eps = torch.tensor(EPS, dtype=torch.float32)
    if rms:
        return torch.zeros(x.shape[0], 1), torch.rsqrt(_sum32(x32 * x32, -1, order)[:, None] / cols + eps)
    mean = _sum32(x32, -1, order)[:, None] / cols
    d = x32 - mean
    return mean, torch.rsqrt(_sum32(d * d, -1, order)[:, None] / cols + eps)


def _emu_norm_fwd(x, w, b, rms, order):
    mean, rstd = _emu_stats(x, rms, order)
    if rms:
        return (w.float() * (x.float() * rstd).to(torch.bfloat16).float()).to(torch.bfloat16)
    y = (x.float() - mean) * rstd * w.float()
    return (y + (b.float() if b is not None else 0.0)).to(torch.bfloat16)


def _emu_norm_bwd(x, w, dy, rms, order, dw_old=None, db_old=None, stats_of=None, dw_rows=None):
    """stats_of: row index whose statistics the LAST row uses (a fault); dw_rows: {column: number of leading rows summed} (a fault)."""
    cols = x.shape[-1]
    mean, rstd = _emu_stats(x, rms, order)
    if stats_of is not None:
        mean, rstd = mean.clone(), rstd.clone()
        mean[-1], rstd[-1] = mean[stats_of], rstd[stats_of]
    xh = (x.float() - mean) * rstd
    g = dy.float() * w.float()
    ma = torch.zeros_like(mean) if rms else _sum32(g, -1, order)[:, None] * (1.0 / cols)
    mb = _sum32(g * xh, -1, order)[:, None] * (1.0 / cols)
    dx = (rstd * (g - ma - xh * mb)).to(torch.bfloat16)
    t = dy.float() * xh
    dw = _sum32(t, 0, order)
    for c, k in (dw_rows or {}).items():
        dw[c] = _sum32(t[:k, c], 0, order)
    dw = (dw + (dw_old.float() if dw_old is not None else 0.0)).to(torch.bfloat16)
    db = (_sum32(dy, 0, order) + (db_old.float() if db_old is not None else 0.0)).to(torch.bfloat16)
    return dx, dw, db


def _emu_ce(z, lab, scale, loss0, order, keep_ignored=False):
    s = torch.tensor(scale, dtype=torch.float32)
    m = z.max(-1, keepdim=True).values
    e = torch.exp(z - m)
    tot = _sum32(e, -1, order)[:, None]
    p = e * (1.0 / tot)
    valid = (lab != -100)[:, None]
    onehot = torch.zeros_like(p).scatter_(1, lab.clamp_min(0)[:, None], 1.0)
    d = torch.where(valid | keep_ignored, (p - onehot * valid) * s, torch.zeros_like(p)).to(torch.bfloat16)
    rows = torch.where(valid, (m + tot.log() - z.gather(1, lab.clamp_min(0)[:, None])) * s, torch.zeros_like(m))
    return d, float(torch.tensor(loss0, dtype=torch.float32) + _sum32(rows[:, 0], 0, order))


def _k(v):
    return torch.tensor(v, dtype=torch.float32)


def _emu_sig(u):
    return 1.0 / (1.0 + torch.exp(-u))


def _emu_acts(z, dy, da):
    x, d, a = z.float(), dy.float(), da.float()
    u2 = 2.0 * _k(GELU_K0) * (x + _k(GELU_K1) * x * x * x)
    s = _emu_sig(u2)
    t = 2.0 * s - 1.0
    er = torch.erf(x * _k(ERF_C))
    sg = _emu_sig(x)
    out = {"fwd1": x * s, "fwd2": 0.5 * x * (1.0 + er),
           "bwd1": d * (0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _k(GELU_K0) * (1.0 + 3.0 * _k(GELU_K1) * x * x)),
           "bwd2": d * (0.5 * (1.0 + er) + x * _k(PDF_C) * torch.exp(-0.5 * x * x)),
           "silu_mul": (x * sg).to(torch.bfloat16).float() * d,
           "dg": a * d * (sg * (1.0 + x * (1.0 - sg))), "du": a * (x * sg)}
    return {k: v.to(torch.bfloat16) for k, v in out.items()}


def _emu_adamw(p, m, v, g, lr, b1, b2, eps, wd, step, gs, skip=None):
    lr, b1, b2, eps, wd, gs = (_k(a) for a in (lr, b1, b2, eps, wd, gs))
    bc1, bc2 = 1.0 - torch.pow(b1, float(step)), 1.0 - torch.pow(b2, float(step))
    gg = g.float() * gs
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    p1 = p * (1.0 - lr * wd)
    p1 = p1 - lr * (m1 / bc1) / (torch.sqrt(v1 / bc2) + eps)
    if skip is not None:
        p1, m1, v1 = p1.clone(), m1.clone(), v1.clone()
        p1[skip], m1[skip], v1[skip] = p[skip], m[skip], v[skip]
    return p1, m1, v1


# ---- the bounds admit the emulations and stay sharp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", NORM_FWD_COLS)
def test_norm_forward_bound_admits_fp32_and_stays_sharp(cols):
    for rows in NORM_FWD_ROWS:
        for dist in NORM_DISTS:
            x, w, b, _ = norm_inputs(rows, cols, dist, device="cpu")
            for kind in ("ln", "ln_nob", "rms"):
                bb = b if kind == "ln" else None
                if kind == "rms":
                    ref, bound, acc, near = rmsnorm_fwd_bound(x.double(), w.double(), EPS)
                    if rows * cols >= MIN_COUNT:
                        assert float(near.double().mean()) < 0.01, f"rms [{rows}, {cols}] {dist}: {float(near.double().mean()):.2%} near-tie elements"
                else:
                    ref, bound, acc = layernorm_fwd_bound(x.double(), w.double(), None if bb is None else bb.double(), EPS)
                for order in ORDERS:
                    _admit(_emu_norm_fwd(x, w, bb, kind == "rms", order), ref, bound, f"{kind} [{rows}, {cols}] {dist} order {order}")
                want = SHARP_EXCEPTIONS["offset"] if (dist == "offset" and kind != "rms") else SHARP_MIN
                if rows * cols >= MIN_COUNT:
                    assert _sharp(ref, acc) >= want, f"{kind} [{rows}, {cols}] {dist}: sharp for {_sharp(ref, acc):.2%}"


@pytest.mark.parametrize("rms,cols,align", NORM_BWD_CASES, ids=lambda v: str(v))
def test_norm_backward_bound_admits_fp32_and_stays_sharp(rms, cols, align):
    for rows in NORM_BWD_ROWS:
        x, w, _, dy = norm_inputs(rows, cols, "wide", seed=1, device="cpu")
        route = norm_bwd_route(rows, cols, rms, aligned=(align == "aligned"))
        old = randn_bf16(cols, seed=rows, scale=2.0, device="cpu")
        for accumulate in (False, True):
            o64 = old.double() if accumulate else None
            want = norm_bwd_bounds(x.double(), w.double(), dy.double(), EPS, rms, route, o64, o64)
            for order in ORDERS:
                got = dict(zip(("dx", "dw", "db"), _emu_norm_bwd(x, w, dy, rms, order, old if accumulate else None, old if accumulate else None)))
                for name, (ref, bound, acc) in want.items():
                    _admit(got[name].reshape(ref.shape)[None] if ref.dim() == 1 else got[name], ref[None] if ref.dim() == 1 else ref, bound[None] if ref.dim() == 1 else bound,
                           f"{'rms' if rms else 'ln'} bwd [{rows}, {cols}] acc={accumulate} order {order} {name}")
            if cols >= MIN_COUNT:
                for name, (ref, _, acc) in want.items():
                    floor = SHARP_MIN if (name == "dx" or rows < 25) else SHARP_EXCEPTIONS["colsum"]
                    assert _sharp(ref, acc) >= floor, f"{name} [{rows}, {cols}] rms={rms} acc={accumulate}: sharp for {_sharp(ref, acc):.2%}"


@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_bound_admits_fp32_and_stays_sharp(V):
    scale, loss0 = 1.0 / 29.0, 1.5
    for rows in ([3] if V == 152064 else CE_ROWS):
        for kind in CE_KINDS:
            z, lab = ce_inputs(rows, V, kind, device="cpu")
            dref, dbound, dacc, loss_ref, loss_bound = ce_bounds(z.double(), lab, scale, loss0)
            for order in ORDERS:
                d, loss = _emu_ce(z, lab, scale, loss0, order)
                _admit(d, dref, dbound, f"ce [{rows}, {V}] {kind} order {order}")
                assert abs(loss - loss_ref) <= loss_bound, (rows, V, kind, loss, loss_ref, loss_bound)
            # the label's own element is p - 1, a cancellation by nature wherever p ~ 1: the criterion is taken over the other elements of the live rows
            plain = (lab != -100)[:, None] & (torch.arange(V)[None, :] != lab[:, None])
            if int(plain.sum()) >= MIN_COUNT:
                assert _sharp(dref[plain], dacc[plain]) >= SHARP_MIN, f"ce [{rows}, {V}] {kind}: sharp for {_sharp(dref[plain], dacc[plain]):.2%}"


def _act_cases():
    for kind in ("sweep", "big"):
        z, dy, da = act_inputs(kind, device="cpu")
        if kind == "big":
            keep = torch.cat([torch.arange(1 << 17), torch.arange(ACT_BIG_N - (1 << 17), ACT_BIG_N)])
            z, dy, da = z[keep], dy[keep], da[keep]
        yield kind, z, dy, da


def test_activation_bounds_admit_fp32_and_stay_sharp():
    for kind, z, dy, da in _act_cases():
        z64, dy64, da64 = z.double(), dy.double(), da.double()
        got = _emu_acts(z, dy, da)
        (rg, bg, ag), (ru, bu, au) = silu_mul_bwd_bound(z64, dy64, da64)
        rs, bs, as_, near = silu_mul_fwd_bound(z64, dy64)
        assert float(near.double().mean()) < 0.01
        table = {"fwd1": gelu_tanh_fwd_bound(z64), "fwd2": gelu_erf_fwd_bound(z64), "bwd1": gelu_tanh_bwd_bound(z64, dy64),
                 "bwd2": gelu_erf_bwd_bound(z64, dy64), "silu_mul": (rs, bs, as_), "dg": (rg, bg, ag), "du": (ru, bu, au)}
        # sharpness where the function is not saturated: the erf form's 1 + erf cancels to an absolute error 13 * 2^-24 (1 + |erf|) by nature, which
        # outweighs the rounding 2^-8 (1 + erf) once 1 + erf < 26 * 2^-16, that is below z = -3.55 (and the derivatives likewise further out), so
        # every case is judged on |z| <= 3.5
        core = z64.abs() <= 3.5
        for name, (ref, bound, acc) in table.items():
            w = _admit(got[name][None], ref[None], bound[None], f"{name} {kind}")
            print(f"{name} {kind}: worst err / bound {w:.3f}, sharp for {_sharp(ref[core], acc[core]):.2%}")
            assert _sharp(ref[core], acc[core]) >= SHARP_MIN, f"{name} {kind}: sharp for {_sharp(ref[core], acc[core]):.2%}"


@pytest.mark.parametrize("n", ADAMW_N + [8192])
def test_adamw_bound_admits_fp32(n):
    """n = 8192: the windows of the launch-seam case (random state; the bound is per element)."""
    p, m, v, g = adamw_state(n, device="cpu")
    for step in ADAMW_STEPS + [3]:
        for wd in (0.0, 0.1):
            for gs in (1.0, 0.37):
                want = adamw_bounds(p.double(), m.double(), v.double(), g.double(), wd=wd, step=step, grad_scale=gs, **ADAMW_HP)
                got = _emu_adamw(p, m, v, g, wd=wd, step=step, gs=gs, **ADAMW_HP)
                for t, (name, (ref, bound)) in zip(got, want.items()):
                    _admit(t[None], ref[None], bound[None], f"adamw n={n} step={step} wd={wd} gs={gs} {name}")


def test_exact_references_on_small_cases():
    """scatter_add_rows_ref against a hand-computed case and depth_to_space_index_map against the kernel's own index formula (train.hip:621-633)."""
    src = torch.tensor([[1.0, 256.0], [1.0, 1.0], [1.0, 1.0]]).to(torch.bfloat16)
    dst = torch.tensor([[256.0, 1.0], [3.0, 3.0]]).to(torch.bfloat16)
    out = scatter_add_rows_ref(src, dst, torch.tensor([0, 1, 0], dtype=torch.int32))
    # row 0: 256 + (1 + 1) = 258 in fp32, rounded once (a per-add rounding would leave 256); 1 + (256 + 1) = 258
    assert out.tolist() == [[258.0, 258.0], [4.0, 4.0]]
    for g, k in D2S_GK:
        gd = (g + k - 1) // k
        pos = depth_to_space_index_map(2, g, k)
        b, sy, sx = torch.meshgrid(torch.arange(2), torch.arange(g), torch.arange(g), indexing="ij")
        want = ((b * gd * gd + (sy // k) * gd + sx // k) * k * k + (sy % k) * k + sx % k).reshape(2, g * g)
        assert torch.equal(pos, want), (g, k)


# ---- the bounds reject the injected faults, three of which the rel-L2 assertions pass ----------------------------------------------------------------
def _rejects(out, ref, bound, what):
    with pytest.raises(AssertionError, match="over the bound|non-finite"):
        assert_elementwise(out, ref, bound, what)


def test_norm_backward_faults_pass_rel_l2_and_fail_the_bound():
    """On the inputs of tests/test_gpu_train.py::test_norm_backward at (64, 3584), RMSNorm (the wave kernel: row blocks of 12, the last one rows 60-63)."""
    rows, cols = 64, 3584
    x = randn_bf16(rows, cols, seed=9, scale=1.5, device="cpu") + 0.3
    w = randn_bf16(cols, seed=10, scale=0.1, device="cpu") + 1
    dy = randn_bf16(rows, cols, seed=12, device="cpu")
    want = norm_bwd_bounds(x.double(), w.double(), dy.double(), EPS, True, norm_bwd_route(rows, cols, True))
    dx, dw, _ = _emu_norm_bwd(x, w, dy, True, 1)
    assert assert_elementwise(dx, *want["dx"][:2], "clean dx") <= 1.0 and assert_elementwise(dw[None], want["dw"][0][None], want["dw"][1][None], "clean dw") <= 1.0
    _, bad_dw, _ = _emu_norm_bwd(x, w, dy, True, 1, dw_rows={cols - 5: 60})
    print(f"one dw column without its last row block: rel-L2 {rel_l2(bad_dw, want['dw'][0]):.3e}")
    assert rel_l2(bad_dw, want["dw"][0]) < 1e-2
    _rejects(bad_dw[None], want["dw"][0][None], want["dw"][1][None], "dw column without its last row block")
    bad_dx, _, _ = _emu_norm_bwd(x, w, dy, True, 1, stats_of=rows - 2)
    print(f"last row's dx with the previous row's statistics: rel-L2 {rel_l2(bad_dx, want['dx'][0]):.3e}")
    assert rel_l2(bad_dx, want["dx"][0]) < 1e-2
    _rejects(bad_dx, *want["dx"][:2], "last row's dx with the previous row's statistics")
    assert not torch.equal(bad_dx[-1], dx[-1]) and torch.equal(bad_dx[:-1], dx[:-1])


def test_layernorm_fault_passes_rel_l2_and_fails_the_bound():
    """On the inputs of tests/test_gpu_ops.py::test_layernorm_rmsnorm at (3, 16384): b dropped on the 8-column chunk whose mean |b| is nearest 0.05 (a
    small bias: 12 times the bound of an output of size 1)."""
    rows, cols = 3, 16384
    x = randn_bf16(rows, cols, seed=14, scale=2.0, device="cpu") + 0.5
    w = randn_bf16(cols, seed=15, scale=0.1, device="cpu") + 1
    b = randn_bf16(cols, seed=16, scale=0.1, device="cpu")
    ref, bound, _ = layernorm_fwd_bound(x.double(), w.double(), b.double(), EPS)
    out = _emu_norm_fwd(x, w, b, False, 1)
    assert assert_elementwise(out, ref, bound, "clean") <= 1.0
    ch = int((b.float().abs().view(-1, 8).mean(-1) - 0.05).abs().argmin())
    bad = out.clone()
    bad[:, ch * 8:ch * 8 + 8] = _emu_norm_fwd(x, w, None, False, 1)[:, ch * 8:ch * 8 + 8]
    print(f"LayerNorm without b on chunk {ch}: rel-L2 {rel_l2(bad, ref):.3e}")
    assert rel_l2(bad, ref) < 3e-3
    _rejects(bad, ref, bound, "LayerNorm without b on one chunk")


def test_the_other_faults_fail_their_checks():
    z, lab = ce_inputs(5, 257, "x3", device="cpu")
    dref, dbound, _, _, _ = ce_bounds(z.double(), lab, 1.0 / 29.0, 1.5)
    assert bool((lab == -100).any())
    _rejects(_emu_ce(z, lab, 1.0 / 29.0, 1.5, 0, keep_ignored=True)[0], dref, dbound, "an ignored label's row not zeroed")
    # a duplicate id added twice: the reference is exact, any difference is a failure
    n, H = 50, 512
    src, table = randn_bf16(n, H, seed=1, device="cpu"), randn_bf16(n + 3, H, seed=2, scale=2.0, device="cpu")
    ids = scatter_ids(n, n + 3, "mixed")
    twice = torch.cat([ids, ids[-1:]])
    assert not torch.equal(scatter_add_rows_ref(src, table, ids), scatter_add_rows_ref(torch.cat([src, src[-1:]]), table, twice))
    # AdamW: the odd tail (element 2 * n2) of n = 4123 skipped, and the first element behind the 2^29 seam of the seam case's middle window
    for n, skip in ((4123, 4122), (2048 + 11, 2048)):
        p, m, v, g = adamw_state(n, seed=skip, device="cpu")
        want = adamw_bounds(p.double(), m.double(), v.double(), g.double(), wd=0.1, step=3, grad_scale=0.37, **ADAMW_HP)
        for t, (name, (ref, bound)) in zip(_emu_adamw(p, m, v, g, wd=0.1, step=3, gs=0.37, skip=skip, **ADAMW_HP), want.items()):
            _rejects(t[None], ref[None], bound[None], f"adamw element {skip} skipped: {name}")
    assert ADAMW_SEAM_N - (1 << 29) == 11


def test_flat_frame_flags_writes_on_both_sides():
    for off, word in ((10, "past"), (-1, "before")):
        view, check = framed_flat(10, torch.float32, device="cpu", fill=torch.zeros(10))
        check()
        view.as_strided((1,), (1,), view.storage_offset() + off).fill_(0.0)
        with pytest.raises(AssertionError, match=word):
            check()

"""The exact regime, the generic bound and the references of tests/test_gpu_w4_elements.py, proved on the CPU before they judge the W4A16 kernels.

A model of the kernels' arithmetic in fp32 (_emulate): per 128-wide group D = the sum of x (128 + q) over 16 chunks of 8, S = the group sum of x,
T = D - (128 + zero) S, and total = fmaf(scale, T, total) along a wave's contiguous range of groups; the W partials are added in wave order.  Three
orders: "forward" (W as the launcher picks it, chunks and groups ascending), "reversed" (chunks, groups and partials descending) and "dealt" (the
groups dealt round-robin to 16 partials).  An output's arithmetic depends on K and on its own weight row alone, so every K of the GPU file is
run on a matrix of 48 rows; N, n and M of the GPU shapes decide which tile, block or slab computes an element, not how.

  - Exactness: on w4_exact_case inputs the three orders give IDENTICAL bits and equal the fp64 product, for every K of the GPU file, both scale
    sets, x_max = 4 and the normed variant (whose staged activation is modelled in fp32 with rstd off by +-4 ulp and comes out as x_eff).
  - Generic bound: two orders stay inside w4_generic_bound at every element of every K of the GPU file (plain with and without bias and residual,
    an activation with mean 3, the fused norm, gate/up).  Measured here: the worst err / bound of the model, and the median over the elements of
    (accumulation term) / (2^-8 |ref|) for Gaussian x and sigma_w = 0.03:
        K       128   256   384   896   1024  1152  1920  2560  3584  6400  13568  14336  14464  18944  20608  24704  32768
        worst   0.66  0.48  0.37  0.27  0.39  0.40  0.27  0.22  0.22  0.18  0.11   0.10   0.11   0.10   0.08   0.09   0.08
        median  2.4   3.7   4.3   6.3   6.6   6.5   10.6  12.1  13.0  15.5  22.9   22.1   27.7   26.1   34.0   32.4   36.8
    So the accumulation term is 2.4 x the cost of one bf16 rounding at K = 128 and 37 x at K = 32768: never dequantising is paid for with a
    worst-case term of 129 * 2^-24 times sums of |x| (128 + q) s, about 135 / |q - z| times what a dequantising kernel's would be, and a correct
    kernel uses a tenth of it at large K.  The generic regime is therefore the coarse net (indexing, tiles, slabs); the exact regime is the fine one.
  - Injected faults (test_injected_faults, test_injected_epilogue_faults), N = 3584 outputs, K = 128 / 1024 / 3584.  Every one is rejected in the
    exact regime (plain outputs: by the bits; 6 and 7: by the bound without accumulation term).  "generic": does w4_generic_bound reject it;
    "rel-L2": the figure today's tests would have seen on the same data (one [N] vector; fault 8 a [16, N] matrix), a correct kernel giving 1.7e-3:
        fault                                                     generic at 128 / 1024 / 3584     rel-L2 at 128 / 1024 / 3584
        1 one word's nibbles read in 0, 1, 2, .. order            yes / yes / NO                   2.0e-3 / 1.7e-3 / 1.7e-3
        2 scale and zero of row n from row n ^ 1 in one group     yes / yes / yes                  1.8e-3 / 5.8e-3 / 1.8e-3
        3 zero off by one in one group of one row                 yes / yes / yes                  1.7e-3 / 2.9e-3 / 3.3e-3
        4 a wave's range ends one group early (one tile)          yes / yes / yes                  1.6e-2 / 1.3e-2 / 1.1e-2
        5 the last tile's rows taken from the previous tile       yes / yes / yes                  3.6e-2 / 6.5e-2 / 8.2e-2
        6 gate and up swapped                                     yes / yes / yes                  above 1.5e-2
        7 RoPE biases e0 / e1 swapped; the sine's sign flipped    yes / yes / yes                  (no rel-L2 test of these kernels existed)
        8 one K slab of <= 8 dropped for one 16 x 16 tile         yes / yes / yes                  2.0e-2 / 1.8e-2 / 2.1e-2
        9 the residual added before the first rounding            NO / NO / NO                     1.7e-3 / 1.7e-3 / 1.7e-3
    Faults 2 and 3 sit in the group where the activations of the row do not cancel (a zero point acts through the group's sum of x); with x of
    mean 0 they move one element of 3584 and no rel-L2 limit sees them.  Faults 1, 2, 3 and 9 pass 1e-2, 1.5e-2 and 3e-2.  Faults 4 and 8 do NOT
    pass 1e-2 on this data, by a little: one group of 28 missing in 16 of 3584 rows is sqrt(16 / (28 * 3584)) = 1.3e-2, a slab of an eighth of K
    in a 16 x 16 tile of [16, 3584] is sqrt(256 / (8 * 16 * 3584)) = 2.4e-2; both pass the 3e-2 of the model-level tests that judge the q|k|v
    kernels, and fault 4 passes 1e-2 from K = 7168 on (6e-3 at K = 14336).  Only the exact regime catches fault 9 (the order of the residual's
    two roundings moves an element by one bf16 spacing, which every bound allows) and, at K = 3584, fault 1 (two weights of eight traded places:
    below the accumulation term there)."""
import functools

import pytest
import torch

from tests.gpu_util import (BF16_U, assert_bits_equal, assert_elementwise, rel_l2, rope_table, w4_exact_case, w4_exact_plain_ref,
                            w4_generic_acc, w4_generic_bound, w4_staged_norm, w4_unpack)
from tests.test_batch_gemm_bound_cpu import _gateup_model, _qkv_model
from tests.test_gpu_w4_elements import (BATCH_DEEP, BATCH_QKV_KS, BATCH_SMALL, BATCH_TILES, BATCH_WALK, PREFILL_KS, SCALE_SETS, SOLO_KS, SOLO_LDS, SOLO_PIPE,
                                        SOLO_QKV_KS, X_MAX)

ALL_KS = sorted({*SOLO_KS, SOLO_PIPE[1], SOLO_LDS[1], *SOLO_QKV_KS, *(k for _, _, k in BATCH_SMALL), *(k for _, _, k in BATCH_TILES), *(k for _, _, k in BATCH_WALK),
                 BATCH_DEEP[2], *BATCH_QKV_KS, *PREFILL_KS, 256})
ORDERS = ("forward", "reversed", "dealt")


def _solo_waves(G):
    """launch_gemv_w4: W = ceil(G / UB) capped at 16."""
    return min(16, -(-G // (10 if G > 112 else 7)))


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product of a bf16 scale and an fp32 value has 32 significant bits, exact in fp64; one rounding to fp32 follows (the
    fp64 addition itself rounds at 2^-53, far below the half-ulp of fp32 except at an exact tie)."""
    return (a.double() * b.double() + c.double()).float()


def _emulate(x, q, zero, scale, order="forward", W=None, skip=None, slab_drop=None):
    """x [n, K] bf16 values as fp32; q [N, K], zero / scale [N, G] as fp32 (scale a bf16 value) -> [n, N] fp32, the kernels' sum before the
    epilogue.  skip = (wave, tile): that wave's range ends one group early for the 16 rows of the tile (fault 4); slab_drop = (splits, slice, rows,
    cols): the K range split like gemm_w4's slices, that slice's contribution missing in the [rows, cols] block (fault 8)."""
    n, K = x.shape
    N, G = zero.shape
    x4, q4 = x.view(n, G, 16, 8), (128.0 + q).view(N, G, 16, 8)
    chunks = torch.einsum("ngce,mgce->nmgc", x4, q4)                      # [n, N, G, 16]: 8 exact products each, summed in fp32
    xs = x4.sum(-1)                                                        # [n, G, 16]
    ch = range(15, -1, -1) if order == "reversed" else range(16)
    D, S = torch.zeros((n, N, G)), torch.zeros((n, G))
    for c in ch:
        D, S = D + chunks[..., c], S + xs[..., c]
    T = D - (128.0 + zero)[None] * S[:, None, :]                            # [n, N, G]: the product rounds, then the difference
    if order == "dealt":
        parts = [list(range(w, G, 16)) for w in range(16)]
    elif slab_drop is not None:
        sp = slab_drop[0]
        parts = [list(range(G * s // sp, G * (s + 1) // sp)) for s in range(sp)]
    else:
        W = _solo_waves(G) if W is None else W
        parts = [list(range(G * w // W, G * (w + 1) // W)) for w in range(W)]
    if order == "reversed":
        parts = [p[::-1] for p in parts][::-1]
    total = torch.zeros((n, N))
    for w, groups in enumerate(parts):
        part = torch.zeros((n, N))
        for i, g in enumerate(groups):
            nxt = _fma32(scale[None, :, g], T[..., g], part)
            if skip is not None and w == skip[0] and i == len(groups) - 1:
                t0 = skip[1] * 16
                nxt[:, t0:t0 + 16] = part[:, t0:t0 + 16]
            part = nxt
        if slab_drop is not None and w == slab_drop[1]:
            part[slab_drop[2], slab_drop[3]] = 0.0
        total = total + part
    return total


def _plain_epilogue(v, bias, res, res_first=False):
    """gemv_w4.hip:233-235 on fp32 v [n, N] -> bf16.  res_first (fault 9): the residual joins before the first rounding."""
    if bias is not None:
        v = v + bias.float()
    if res is not None:
        v = (v + res.float()) if res_first else v.to(torch.bfloat16).float() + res.float()
    return v.to(torch.bfloat16)


def _staged_f32(x, norm_w, eps, ulps):
    """stage_x_w4 with a fused norm in fp32 (gemv_w4.hip:63-71), rstd moved by `ulps` fp32 spacings: what rsqrtf, the division and the order of the
    sum may do to it."""
    xf = x.float()
    tot = (xf * xf).sum(-1, keepdim=True)
    rstd = torch.rsqrt(tot / x.shape[1] + torch.tensor(eps, dtype=torch.float32))
    rstd = rstd * (1.0 + ulps * 2.0 ** -23)
    return (norm_w.float() * (xf * rstd).to(torch.bfloat16).float()).to(torch.bfloat16)


def _unpacked(mat, gateup=False):
    q, z, s = (t.float() for t in w4_unpack(mat.logical))
    return ((q[0::2], z[0::2], s[0::2]), (q[1::2], z[1::2], s[1::2])) if gateup else (q, z, s)


# ---- the exact regime's premise -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normed", [False, True], ids=["plain", "normed"])
@pytest.mark.parametrize("scales", SCALE_SETS, ids=str)
@pytest.mark.parametrize("K", ALL_KS)
def test_exact_regime_is_order_independent(K, scales, normed):
    c = w4_exact_case(48, K, K + len(ALL_KS), scales, X_MAX, rows=2, normed=normed)
    q, z, s = _unpacked(c["mat"])
    if normed:
        for ulps in (-4, 0, 4):
            assert torch.equal(_staged_f32(c["x"], c["norm_w"], c["eps"], ulps), c["x_eff"]), f"the staged activation is not +-norm_w at {ulps} ulp of rstd"
        staged, slack = w4_staged_norm(c["x"].double(), c["norm_w"].double(), c["eps"])
        assert torch.equal(staged, c["x_eff"]) and float(slack.max()) == 0.0
    x = c["x_eff"].float()
    sums = [_emulate(x, q, z, s, order) for order in ORDERS]
    for order, v in zip(ORDERS[1:], sums[1:]):
        assert torch.equal(v.view(torch.int32), sums[0].view(torch.int32)), f"K = {K}: the {order} order differs from the forward one"
    assert torch.equal(sums[0].double(), c["core"]), f"K = {K}: the fp32 sum is not the fp64 product"
    for bias, res in ((None, None), (c["bias"], None), (c["bias"], c["res"])):
        b64, r64 = None if bias is None else bias.double(), None if res is None else res.double()
        assert_bits_equal(_plain_epilogue(sums[0], bias, res), w4_exact_plain_ref(c["core"], b64, r64), f"K = {K} exact plain")


# ---- the generic bound ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic(N, K, seed, gateup=False, mean_x=0.0, rows=2):
    from vila_amd.quant import W4Matrix
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.03
    mat = W4Matrix.pack(w, torch.randn(N, K, generator=g) * 0.03 if gateup else None)
    x = (mean_x + torch.randn(rows, K, generator=g)).to(torch.bfloat16)
    return dict(mat=mat, x=x, bias=torch.randn(N, generator=g).to(torch.bfloat16), res=torch.randn(rows, N, generator=g).to(torch.bfloat16),
                norm_w=(1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16))


@pytest.mark.parametrize("K", ALL_KS)
def test_generic_bound_holds_for_the_model(K):
    """Two orders inside the bound at every element, plain (with bias and residual), gate/up, and with the fused norm (the model's rstd off by
    +-4 ulp); an activation with a large mean (the cancellation of tests/test_gpu_w4.py::test_gemv_w4_large_offsets_cancel) as well."""
    worst = 0.0
    for mean_x in (0.0, 3.0):
        p = _generic(48, K, K, mean_x=mean_x)
        q, z, s = _unpacked(p["mat"])
        core, acc = w4_generic_acc(p["x"].double(), q.double(), z.double(), s.double())
        for order in ("forward", "dealt"):
            v = _emulate(p["x"].float(), q, z, s, order)
            for bias, res in ((None, None), (p["bias"], p["res"])):
                b64, r64 = None if bias is None else bias.double(), None if res is None else res.double()
                ref, bound = w4_generic_bound("plain", K, core, acc, bias64=b64, res64=r64)
                worst = max(worst, assert_elementwise(_plain_epilogue(v, bias, res), ref, bound, f"K = {K} {order} mean {mean_x}"))
    p = _generic(48, K, K)
    q, z, s = _unpacked(p["mat"])
    staged, slack = w4_staged_norm(p["x"].double(), p["norm_w"].double(), 1e-6)
    core, acc = w4_generic_acc(staged.double(), q.double(), z.double(), s.double(), slack)
    for ulps in (-4, 4):
        v = _emulate(_staged_f32(p["x"], p["norm_w"], 1e-6, ulps).float(), q, z, s)
        worst = max(worst, assert_elementwise(_plain_epilogue(v, None, None), *w4_generic_bound("plain", K, core, acc), f"K = {K} normed, rstd {ulps} ulp"))
    p = _generic(24, K, K + 1, gateup=True)
    (qg, zg, sg), (qu, zu, su) = _unpacked(p["mat"], True)
    cg, ag = w4_generic_acc(p["x"].double(), qg.double(), zg.double(), sg.double())
    cu, au = w4_generic_acc(p["x"].double(), qu.double(), zu.double(), su.double())
    ref, bound = w4_generic_bound("gateup", K, cg, ag, cu, au)
    for order in ("forward", "dealt"):
        out = _gateup_model(_emulate(p["x"].float(), qg, zg, sg, order), _emulate(p["x"].float(), qu, zu, su, order))
        worst = max(worst, assert_elementwise(out, ref, bound, f"K = {K} gate/up {order}"))
    ratio = float((acc / (BF16_U * core.abs()).clamp_min(1e-300)).median())
    print(f"K = {K}: worst err / bound of the model {worst:.4f}; median accumulation term / (2^-8 |ref|) {ratio:.2f}")
    assert worst <= 1.0


# ---- injected faults ------------------------------------------------------------------------------------------------------------------------------------------
def _nibble_fault(q, row, word):
    """Fault 1: the 8 weights of one word read in nibble order 0, 1, 2, .. where nibble p < 4 holds element 2 p and nibble p + 4 element 2 p + 1."""
    q = q.clone()
    e = q[row, word * 8:word * 8 + 8].clone()
    nib = torch.stack((e[0::2], e[1::2])).reshape(-1)                       # the word's nibbles 0 .. 7
    q[row, word * 8:word * 8 + 8] = nib
    return q


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


FAULT_KS = (128, 1024, 3584)
N_BIG = 3584


@functools.lru_cache(maxsize=None)
def _fault_data(K, regime):
    """N = 3584 outputs at K: (x [16, K] fp32, (q, z, s), bias, res, core, acc, good sums)."""
    if regime == "exact":
        c = w4_exact_case(N_BIG, K, 77 + K, SCALE_SETS[0], X_MAX, rows=16)
        x, mat, bias, res, core = c["x"].float(), c["mat"], c["bias"], c["res"], c["core"]
        q, z, s = _unpacked(mat)
        acc = torch.zeros_like(core)
    else:
        p = _generic(N_BIG, K, 78 + K, rows=16)
        x, mat, bias, res = p["x"].float(), p["mat"], p["bias"], p["res"]
        q, z, s = _unpacked(mat)
        core, acc = w4_generic_acc(x.double(), q.double(), z.double(), s.double())
    return x, (q, z, s), bias, res, core, acc


def _plain_verdicts(K, regime, bad_sums=None, bad_out=None, use_res=False, rows=slice(0, 1)):
    """-> (rejected by the regime's own check, rel-L2 of the faulty output against the reference) for a plain epilogue with bias (and residual)."""
    x, _, bias, res, core, acc = _fault_data(K, regime)
    r = res[rows] if use_res else None
    out = bad_out if bad_out is not None else _plain_epilogue(bad_sums, bias, r)
    b64, r64 = bias.double(), None if r is None else r.double()
    if regime == "exact":
        rej = _rejected(lambda: assert_bits_equal(out, w4_exact_plain_ref(core[rows], b64, r64), "fault"))
        ref = core[rows] + b64 + (0.0 if r64 is None else r64)
    else:
        ref, bound = w4_generic_bound("plain", K, core[rows], acc[rows], bias64=b64, res64=r64)
        rej = _rejected(lambda: assert_elementwise(out, ref, bound, "fault"))
    return rej, rel_l2(out, ref)


@pytest.mark.parametrize("K", FAULT_KS)
def test_injected_faults(K):
    """Every fault of the module docstring's table: rejected in the exact regime; the generic bound's verdict and the rel-L2 figures as the table
    states them (the inequalities below)."""
    G, verdict = K // 128, {}
    for regime in ("exact", "generic"):
        x, (q, z, s), bias, res, core, acc = _fault_data(K, regime)
        x1 = x[:1]
        good = _emulate(x1, q, z, s)
        ok, rel0 = _plain_verdicts(K, regime, bad_sums=good)
        assert not ok and rel0 < 4e-3, (K, regime, "the model itself", rel0)
        # a wrong zero point or scale acts through the group's sum of activations: the faults sit in the group where row 0's do not cancel
        row, grp = 1234, int(x1.view(G, 128).sum(-1).abs().argmax())
        # 1: nibble order of one word.  (A word whose eight nibbles are already in that order is no fault: take the first that is not.)
        word = next(w for w in range(G // 2 * 16, K // 8) if not torch.equal(_nibble_fault(q, row, w), q))
        verdict[1, regime] = _plain_verdicts(K, regime, bad_sums=_emulate(x1, _nibble_fault(q, row, word), z, s))
        # 2: scale and zero of row n from row n ^ 1 in one group
        z2, s2 = z.clone(), s.clone()
        z2[row, grp], s2[row, grp] = z[row ^ 1, grp], s[row ^ 1, grp]
        assert (z2[row, grp], s2[row, grp]) != (z[row, grp], s[row, grp])
        verdict[2, regime] = _plain_verdicts(K, regime, bad_sums=_emulate(x1, q, z2, s2))
        # 3: zero off by one in one group of one row
        z3 = z.clone()
        z3[row, grp] += 1.0
        verdict[3, regime] = _plain_verdicts(K, regime, bad_sums=_emulate(x1, q, z3, s))
        # 4: a wave's range ends one group early, for the 16 rows of one tile
        verdict[4, regime] = _plain_verdicts(K, regime, bad_sums=_emulate(x1, q, z, s, skip=(0, row // 16)))
        # 5: the last tile's rows taken from the previous tile
        bad = good.clone()
        bad[:, -16:] = good[:, -32:-16]
        verdict[5, regime] = _plain_verdicts(K, regime, bad_sums=bad)
        # 8: one K slab dropped for one 16 x 16 tile of a [16, N] prefill (8 slices where G allows, as gemm_w4's geometry clamps them)
        sp = min(8, G)
        good16 = _emulate(x, q, z, s, slab_drop=(sp, sp, slice(0, 0), slice(0, 0)))
        assert not _plain_verdicts(K, regime, bad_sums=good16, rows=slice(0, 16))[0]
        bad16 = _emulate(x, q, z, s, slab_drop=(sp, sp // 2, slice(0, 16), slice(row // 16 * 16, row // 16 * 16 + 16)))
        verdict[8, regime] = _plain_verdicts(K, regime, bad_sums=bad16, rows=slice(0, 16))
        # 9: the residual added before the first rounding
        assert not _plain_verdicts(K, regime, bad_sums=good, use_res=True)[0]
        verdict[9, regime] = _plain_verdicts(K, regime, bad_out=_plain_epilogue(good, bias, res[:1], res_first=True), use_res=True)
    for f in (1, 2, 3, 4, 5, 8, 9):
        assert verdict[f, "exact"][0], f"fault {f} passes the exact regime at K = {K}"
    print(f"K = {K}: " + "; ".join(f"fault {f}: generic {'rejects' if verdict[f, 'generic'][0] else 'passes'}, rel-L2 {verdict[f, 'generic'][1]:.1e}" for f in (1, 2, 3, 4, 5, 8, 9)))
    # what the table states of the generic bound and of today's rel-L2 limit of 1e-2 on the same data
    for f in (2, 4, 5, 8):
        assert verdict[f, "generic"][0], f"fault {f} passes the generic bound at K = {K}"
    assert not verdict[9, "generic"][0], "the generic bound cannot see the order of the residual's two roundings"
    assert verdict[3, "generic"][0], f"fault 3 passes the generic bound at K = {K}"
    assert verdict[1, "generic"][0] == (K < 3584), "fault 1 is below the accumulation term at K = 3584 and above it at 128 and 1024"
    for f in (1, 2, 3, 9):
        assert verdict[f, "generic"][1] < 1e-2, f"fault {f} would fail today's rel-L2 limit at N = {N_BIG}: {verdict[f, 'generic'][1]:.2e}"
    for f in (4, 8):
        assert 1e-2 < verdict[f, "generic"][1] < 3e-2, f"fault {f}: rel-L2 {verdict[f, 'generic'][1]:.2e}, stated as between the 1e-2 and the 3e-2 limit"
    assert verdict[5, "generic"][1] > 3e-2


@pytest.mark.parametrize("K", FAULT_KS)
def test_injected_epilogue_faults(K):
    """Faults 6 and 7 act in the epilogues whose exact-regime check is a bound with the accumulation term set to zero."""
    heads = (2, 1, 64)
    nq, nkv, hd = heads
    N = (nq + 2 * nkv) * hd
    cs = rope_table([1024], hd)
    for regime in ("exact", "generic"):
        if regime == "exact":
            c = w4_exact_case(N // 2, K, K + 5, SCALE_SETS[1], X_MAX, rows=1, gateup=True)
            x, cg, cu = c["x"].float(), c["core"], c["core_up"]
            (qg, zg, sg), (qu, zu, su) = _unpacked(c["mat"], True)
            ag = au = torch.zeros_like(cg)
        else:
            p = _generic(N // 2, K, K + 6, gateup=True, rows=1)
            x = p["x"].float()
            (qg, zg, sg), (qu, zu, su) = _unpacked(p["mat"], True)
            cg, ag = w4_generic_acc(x.double(), qg.double(), zg.double(), sg.double())
            cu, au = w4_generic_acc(x.double(), qu.double(), zu.double(), su.double())
        vg, vu = _emulate(x, qg, zg, sg), _emulate(x, qu, zu, su)
        ref, bound = w4_generic_bound("gateup", K, cg, ag, cu, au)
        assert assert_elementwise(_gateup_model(vg, vu), ref, bound, f"gate/up {regime}") <= 1.0
        with pytest.raises(AssertionError, match="over the bound"):                                        # 6
            assert_elementwise(_gateup_model(vu, vg), ref, bound, f"gate and up swapped, {regime}")
        assert rel_l2(_gateup_model(vu, vg), ref) > 1.5e-2
        # 7: q|k|v.  The model sums rows in natural order; the packed order is the kernels' business and the GPU file's
        if regime == "exact":
            c = w4_exact_case(N, K, K + 7, SCALE_SETS[0], X_MAX, rows=1)
            x, core, bias = c["x"].float(), c["core"], c["bias"]
            q, z, s = _unpacked(c["mat"])
            acc = torch.zeros_like(core)
        else:
            p = _generic(N, K, K + 8, rows=1)
            x, bias = p["x"].float(), p["bias"]
            q, z, s = _unpacked(p["mat"])
            core, acc = w4_generic_acc(x.double(), q.double(), z.double(), s.double())
        v = _emulate(x, q, z, s)
        ref, bound = w4_generic_bound("qkv", K, core, acc, bias64=bias.double(), cs64=cs.double(), heads=heads)
        assert assert_elementwise(_qkv_model(v, bias, cs, nq, nkv, hd), ref, bound, f"qkv {regime}") <= 1.0
        swapped = bias.clone()                                                                              # e0 <-> e1: the partners' biases trade places
        b4 = swapped[:(nq + nkv) * hd].view(nq + nkv, 2, hd // 2)
        b4.copy_(b4.flip(1).clone())
        with pytest.raises(AssertionError, match="over the bound"):
            assert_elementwise(_qkv_model(v, swapped, cs, nq, nkv, hd), ref, bound, f"RoPE partner biases swapped, {regime}")
        flipped = cs.clone()
        flipped[:, hd // 2:] *= -1.0
        with pytest.raises(AssertionError, match="over the bound"):
            assert_elementwise(_qkv_model(v, bias, flipped, nq, nkv, hd), ref, bound, f"sine's sign flipped, {regime}")

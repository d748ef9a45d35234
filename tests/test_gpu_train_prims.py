"""GPU parity tests of the small SFT and prefill primitives (vila_amd/ops.py: colsum, sumsq, rope_table, rope_fwd_, rope_bwd_, im2col, add)
against float64 / exact references on the same bf16 inputs.  Where a kernel does its arithmetic in fp32 and rounds once, the reference repeats
that arithmetic in torch and the test expects bit-equality; the bounds elsewhere are stated per test."""
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import randn_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def _bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """bf16 spacing at |x| (8 significant bits): 2^(e - 8) for |x| = m 2^e, m in [0.5, 1)."""
    _, e = torch.frexp(x.abs().double())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


@pytest.mark.parametrize("C", [8, 136, 1152, 3584])
@pytest.mark.parametrize("R", [1, 127, 129, 8192, 8193, 30000])
def test_colsum_two_stage_matches_fp64(ops, R, C):
    """out[c] (+)= sum_r x[r][c] through <= 64 fp32 partials per column added in a fixed order.  Dense and strided input (ld > C), with and
    without accumulate.  Bound: 1 bf16 ulp of |ref| + 1e-6 * sum |x| per column (the final rounding plus fp32 partial sums); two calls agree
    bit for bit."""
    base = randn_bf16(R, C + 24, seed=R + C)
    prev = randn_bf16(C, seed=7, scale=4.0)
    for x in (base[:, :C].contiguous(), base[:, :C]):                 # ld = C, then ld = C + 24
        for accumulate in (False, True):
            out = prev.clone() if accumulate else torch.full((C,), float("nan"), device="cuda", dtype=torch.bfloat16)
            out2 = out.clone()
            ops.colsum(x, out, accumulate=accumulate)
            ops.colsum(x, out2, accumulate=accumulate)
            assert torch.equal(out, out2), f"R={R} C={C} ld={x.stride(0)} acc={accumulate}: two calls differ"
            xd = x.double()
            ref = xd.sum(0) + (prev.double() if accumulate else 0.0)
            mag = xd.abs().sum(0) + (prev.double().abs() if accumulate else 0.0)
            err = (out.double() - ref).abs()
            bound = _bf16_ulp(ref) + 1e-6 * mag
            bad = (err > bound).nonzero().flatten()
            assert bad.numel() == 0, (f"R={R} C={C} ld={x.stride(0)} acc={accumulate}: {bad.numel()} columns off, first {int(bad[0])}: "
                                      f"got {float(out[bad[0]])} ref {float(ref[bad[0]])}")


@pytest.mark.parametrize("period,C", [(1024, 1152), (3, 8)])
@pytest.mark.parametrize("nrep", [1, 4, 14])
def test_colsum_periodic_is_the_fp32_sum_rounded_once(ops, period, C, nrep):
    """Position-embedding gradient: out[p] (+)= sum_b x[b * period + p], fp32 in image order, the old out added last, one rounding: bit-exact."""
    x = randn_bf16(period * nrep, C, seed=nrep)
    prev = randn_bf16(period, C, seed=11, scale=4.0)
    for accumulate in (False, True):
        out = prev.clone()
        ops.colsum(x, out, accumulate=accumulate, period=period)
        acc = torch.zeros((period, C), device="cuda", dtype=torch.float32)
        for b in range(nrep):
            acc += x[b * period:(b + 1) * period].float()
        if accumulate:
            acc += prev.float()
        assert torch.equal(out, acc.to(torch.bfloat16)), f"period={period} nrep={nrep} acc={accumulate}"


def _sumsq_ref(x: torch.Tensor) -> float:
    tot = 0.0
    flat = x.view(-1)
    step = 1 << 27
    for i in range(0, flat.numel(), step):
        tot += float(flat[i:i + step].double().square().sum())
    return tot


@pytest.mark.parametrize("n", [1, 7, 524288 + 3, 30_000_005, (1 << 31) + 1000])
def test_sumsq_matches_fp64(ops, n):
    """Global grad-norm: <= 2048 block partials added in a fixed order.  n = 2^31 + 1000 (4.3 GB of bf16, an 8B model's flat gradient) needs
    64-bit indexing.  Bound: rel error < 1e-5; two calls agree bit for bit."""
    x = torch.empty((n,), device="cuda", dtype=torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    step = 1 << 28
    for i in range(0, n, step):
        m = min(step, n - i)
        x[i:i + m] = (torch.randn(m, device="cuda", generator=g) * 0.01).to(torch.bfloat16)
    x[n - 1] = 3.0                                                     # the last element must be counted: a 32-bit index would lose it
    got, got2 = ops.sumsq(x), ops.sumsq(x)
    assert torch.equal(got, got2)
    ref = _sumsq_ref(x)
    rel = abs(float(got) - ref) / ref
    assert rel < 1e-5, f"n={n}: sumsq {float(got)} vs fp64 {ref} (rel {rel:.3e})"


# measured on MI355X over the cases below: max |device - HF| = 3.9e-3 (= 2^-8, one bf16 ulp below 1) in both cases; 1.2-1.8 % of the entries
# differ (hd 128: 194 cos / 218 sin of 16 320; hd 64: 124 / 143 of 8160).  Bounds: two bf16 ulps, 5 % of the entries.
ROPE_TABLE_MAX_ABS = 2 * 2 ** -8
ROPE_TABLE_MAX_FLIPS = 0.05


@pytest.mark.parametrize("hd,theta", [(128, 1e6), (64, 1e4)])
def test_rope_table_matches_hf(ops, hd, theta):
    """cos / sin tables against HF's formula: inv_freq = 1 / theta^(arange(0, hd, 2) / hd) in fp32, the angle pos * inv_freq in fp32, cos / sin
    of that angle (fp64 here), rounded to bf16.  The device's powf may differ from torch's by an fp32 ulp, which moves the angle at position
    32767 by up to ~2e-3 rad, and a rounding flip then costs one bf16 ulp (2^-8 below 1).  Measured: ROPE_TABLE_MAX_ABS's comment."""
    pos = torch.cat([torch.tensor([0, 32767, 1, 4095, 4096]), torch.randint(0, 32768, (250,), generator=torch.Generator().manual_seed(hd))])
    pos = pos.to(torch.int32)
    cs, sn = ops.rope_table(pos.cuda(), hd, theta)
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    ang = pos.float()[:, None] * inv[None]
    ref_c = ang.double().cos().to(torch.bfloat16).float()
    ref_s = ang.double().sin().to(torch.bfloat16).float()
    err = max(float((cs.cpu() - ref_c).abs().max()), float((sn.cpu() - ref_s).abs().max()))
    flips = max(float((cs.cpu() != ref_c).double().mean()), float((sn.cpu() != ref_s).double().mean()))
    assert torch.equal(cs.cpu().to(torch.bfloat16).float(), cs.cpu()), "the table holds bf16 values"
    assert err <= ROPE_TABLE_MAX_ABS, f"hd={hd} theta={theta}: max deviation {err:.3e}"
    assert flips < ROPE_TABLE_MAX_FLIPS, f"hd={hd} theta={theta}: {flips:.2%} of the entries differ from HF's"
    assert torch.equal(cs[0].cpu(), torch.ones(hd // 2)) and torch.equal(sn[0].cpu(), torch.zeros(hd // 2)), "position 0"


def _packed_positions(S):
    """non-monotonic positions as in a packed batch: several samples, each counting from 0."""
    if S == 1:
        return torch.tensor([5], dtype=torch.int32, device="cuda")
    return torch.cat([torch.arange(0, 300), torch.arange(0, 200), torch.arange(0, S - 500)]).to(torch.int32).cuda()


def _rot_ref(x1, x2, c, s):
    """HF apply_rotary_pos_emb in bf16 arithmetic: y = bf16(bf16(x * cos) + bf16(rotate_half(x) * sin))."""
    return x1 * c + (-x2) * s, x2 * c + x1 * s


@pytest.mark.parametrize("S", [1, 769])
@pytest.mark.parametrize("nq,nkv,hd", [(28, 4, 128), (16, 2, 64)])
def test_rope_fwd_is_hf_in_bf16(ops, nq, nkv, hd, S):
    """rope_kv_kernel without a cache (the SFT forward; the fused reduce of the prefill is tested bit-equal to it): bit-exact against HF's bf16
    rounding order on the kernel's own tables; the V heads come back bit-unchanged."""
    pos = _packed_positions(S)
    cs, sn = ops.rope_table(pos, hd, 1e6)
    qkv = randn_bf16(S, (nq + 2 * nkv) * hd, seed=S + hd)
    x = qkv.clone()
    ops.rope_fwd_(qkv, cs, sn, pos, nq, nkv, hd)
    half = hd // 2
    qk = x[:, :(nq + nkv) * hd].view(S, nq + nkv, hd)
    c, s = cs.to(torch.bfloat16)[:, None], sn.to(torch.bfloat16)[:, None]
    y1, y2 = _rot_ref(qk[..., :half], qk[..., half:], c, s)
    got = qkv[:, :(nq + nkv) * hd].view(S, nq + nkv, hd)
    assert torch.equal(got[..., :half], y1) and torch.equal(got[..., half:], y2), f"rope_fwd differs in {int((got != torch.cat([y1, y2], -1)).sum())} elements"
    assert torch.equal(qkv[:, (nq + nkv) * hd:], x[:, (nq + nkv) * hd:]), "V heads touched"


@pytest.mark.parametrize("S", [1, 769])
@pytest.mark.parametrize("nq,nkv,hd", [(28, 4, 128), (16, 2, 64)])
def test_rope_bwd_is_the_adjoint(ops, nq, nkv, hd, S):
    """dx1 = bf16(dy1 c + dy2 s), dx2 = bf16(dy2 c - dy1 s) in fp32 (no contraction on either side): bit-exact; V untouched; and
    <rope_fwd(x), y> = <x, rope_bwd(y)> in fp64 up to the bf16 roundings, for a random y and for y = rope_fwd(x)."""
    pos = _packed_positions(S)
    cs, sn = ops.rope_table(pos, hd, 1e6)
    W = (nq + 2 * nkv) * hd
    dy = randn_bf16(S, W, seed=S + hd + 1)
    g = dy.clone()
    ops.rope_bwd_(g, cs, sn, nq, nkv, hd)
    half = hd // 2
    d = dy[:, :(nq + nkv) * hd].view(S, nq + nkv, hd).float()
    c, s = cs[:, None], sn[:, None]
    r1 = (d[..., :half] * c + d[..., half:] * s).to(torch.bfloat16)
    r2 = (d[..., half:] * c - d[..., :half] * s).to(torch.bfloat16)
    got = g[:, :(nq + nkv) * hd].view(S, nq + nkv, hd)
    assert torch.equal(got[..., :half], r1) and torch.equal(got[..., half:], r2), "rope_bwd differs from bf16(dy1 c + dy2 s) / bf16(dy2 c - dy1 s)"
    assert torch.equal(g[:, (nq + nkv) * hd:], dy[:, (nq + nkv) * hd:]), "V part touched"
    x = randn_bf16(S, W, seed=S + hd + 2)
    fx = x.clone()
    ops.rope_fwd_(fx, cs, sn, pos, nq, nkv, hd)
    for y in (randn_bf16(S, W, seed=S + hd + 3), fx.clone()):
        by = y.clone()
        ops.rope_bwd_(by, cs, sn, nq, nkv, hd)
        lhs, rhs = float((fx.double() * y.double()).sum()), float((x.double() * by.double()).sum())
        scale = float(x.double().norm() * y.double().norm())
        assert abs(lhs - rhs) <= 1e-3 * scale, f"<rope(x), y> {lhs} vs <x, rope^T(y)> {rhs} (|x||y| {scale:.3e})"


def _im2col_call(px, P, Kp):
    from vila_amd import _lib
    from vila_amd.ops import _stream
    B, Cc, H, W = px.shape
    out = torch.full((B * (H // P) * (W // P), Kp), float("nan"), device="cuda", dtype=torch.bfloat16)     # the zero tail must be written
    _lib.check(_lib.load().vila_im2col_bf16(px.data_ptr(), out.data_ptr(), B, Cc, H, W, P, Kp, _stream()), "im2col")
    return out


@pytest.mark.parametrize("P,B,H,W,pad", [(14, 1, 448, 448, 0), (14, 14, 448, 448, 4), (16, 1, 384, 384, 0), (16, 14, 224, 224, 32),
                                         (14, 2, 224, 448, 12)])
def test_im2col_is_unfold(ops, P, B, H, W, pad):
    """im2col == F.unfold(px, P, stride=P).transpose(1, 2): columns in (c, ky, kx) order, rows (image, gy, gx), zero-padded to Kp: bit-exact."""
    px = randn_bf16(B, 3, H, W, seed=P + B + pad)
    K = 3 * P * P
    out = _im2col_call(px, P, K + pad)
    ref = F.unfold(px.float().cpu(), P, stride=P).transpose(1, 2).reshape(-1, K)
    ref = torch.cat([ref, torch.zeros(ref.shape[0], pad)], 1).to(torch.bfloat16)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("n", [8, 8 * 1_000_003])
def test_add_is_torch_bf16_add(ops, n):
    a, b = randn_bf16(n, seed=1), randn_bf16(n, seed=2, scale=3.0)
    assert torch.equal(ops.add(a, b), a + b)

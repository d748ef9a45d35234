"""The kernels of the batched step with per-row LoRA adapters, each launched alone in framed buffers against fp64 references.

shrink / expand (vila_amd/csrc/lora_decode.hip, vila_lora_shrink_bf16 / vila_lora_expand_f32): a bank of three slots between NaN guard slots, of
which slot 1 holds NaN and is named by no row (a read of a slot that no row names shows as NaN); x with ldx = K + 8, NaN padding and NaN guard rows;
T and D views of 16 rows, ld + 8, in buffers that hold a bit pattern, only n rows in use: afterwards everything outside the n rows and the Rs / N
columns is the pattern.  Every element is held to bgemm_acc_bound (tests/gpu_util.py) on the scaled products: (1 + 2^-8) (K + 10) 2^-24 sum |s x a|
for shrink — K products, the adds of the 8 wave partials and the scale —, the same with K = r for expand (r products fmaf'ed in order).  Rows
without an adapter are +0.0 bit for bit; T rows of such rows are NaN on the way into expand (they are not read); two calls give the same bits; row
i alone (n = 1) gives the bits of row i of the mixed batch.
Shapes: n in {1, 7, 8, 9, 16}; K in {64 (one k-block: seven of a block's eight waves have none), 576 and 1088 (9 and 17 k-blocks: uneven deals),
3584}; Rs in {16, 48, 192} (1, 3, 12 tiles of 16 adapter rows); expand N in {16, 1000 (N % 16 != 0, a partial last block of 256 columns), 4608},
r in {16, 64}, one segment and three (q | k | v).

The addend entries (decode_batch.hip bgemm_epilogue<ADD>, vila_gemm_batch_lora_bf16 / vila_gateup_batch_lora_bf16 / vila_qkv_batch_lora_bf16): the
three epilogues at n in {1, 8, 9, 16} under bgemm_plain_bound / bgemm_gateup_bound / bgemm_qkv_bound with the core and its absolute sum extended by
D for the rows that add; rows with -1 carry NaN in their addend row and must come out as without it.  With a NULL addend, and with every row -1,
the bits equal those of the entries without addend on the same inputs."""
import pytest
import torch

from tests import lora_serving_ref as R
from tests.lora_serving_ref import assert_bits_equal
from tests.gpu_util import (assert_elementwise, assert_qkv_outputs, bgemm_acc_bound, bgemm_gateup_bound, bgemm_plain_bound, bgemm_qkv_bound,
                            framed_cache, framed_operand, framed_out_rows, rope_table)

pytestmark = pytest.mark.gpu

G = 4
NS = (1, 7, 8, 9, 16)
KS = (64, 576, 1088, 3584)
RSS = (16, 48, 192)
EXPAND_NS = (16, 1000, 4608)
RANKS = (16, 64)
ADD_NS = (1, 8, 9, 16)
MAX_CTX = 8
POS16 = (3, 8, 5, 13, 7, 0, 8, 2, 13, 6, 0, 7, 1, 13, 4, 3)
ROPE_POS16 = (0, 1, 2999, 17, 1024, 3000, 511, 77, 2048, 5, 1500, 333, 2500, 64, 999, 12)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU faulted, nothing more is launched: {e}", returncode=3)


# ---- shrink ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shrink_problems():
    """(K, Rs) -> x of 16 rows and the bank's A, drawn once."""
    cache = {}

    def get(K, Rs):
        if (K, Rs) not in cache:
            cache[(K, Rs)] = (R.rand_bf16((16, K), 11 + K + Rs), R.framed_bank(R.rand_bf16((R.CAPACITY, Rs, K), 13 + K + Rs, K ** -0.5)))
        return cache[(K, Rs)]
    return get


def _shrink_call(ops, x16, a_bank, rows, slots):
    n = len(rows)
    out, check = framed_out_rows(n, a_bank.shape[1], 8, G, dtype=torch.float32)
    ops.lora_shrink(framed_operand(x16[rows], 8, G), a_bank, R.scales(), R.slots_tensor(slots), out)
    _sync()
    return out, check


@pytest.mark.parametrize("Rs", RSS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_shrink_every_element(ops, shrink_problems, n, K, Rs):
    x16, a_bank = shrink_problems(K, Rs)
    rows = list(range(n))
    worst = 0.0
    for kind in R.MAPS:
        slots = R.row_map(kind, n)
        what = f"shrink n={n} K={K} Rs={Rs} [{kind}]"
        out, check = _shrink_call(ops, x16, a_bank, rows, slots)
        ref, ab = R.shrink_ref(x16[:n], a_bank, torch.tensor(R.SCALES, dtype=torch.float32), slots)
        worst = max(worst, assert_elementwise(out[:n], ref, bgemm_acc_bound(ab, K), what))
        check()
        for i, a in enumerate(slots):
            if a < 0:
                assert R.is_plus_zero(out[i]), f"{what}: row {i} has no adapter and is not +0.0"
        again, _ = _shrink_call(ops, x16, a_bank, rows, slots)
        assert_bits_equal(again[:n], out[:n], f"{what}: two calls")
    print(f"shrink ({n}, {K}, {Rs}): worst err / bound {worst:.3f}")


@pytest.mark.parametrize("K,Rs", [(576, 48), (3584, 192)])
def test_shrink_row_alone_equals_row_of_the_mixed_batch(ops, shrink_problems, K, Rs):
    x16, a_bank = shrink_problems(K, Rs)
    for n in (9, 16):
        slots = R.row_map("mixed", n)
        out, _ = _shrink_call(ops, x16, a_bank, list(range(n)), slots)
        for i in range(n):
            solo, check = _shrink_call(ops, x16, a_bank, [i], [slots[i]])
            assert_bits_equal(solo[0], out[i], f"shrink K={K} Rs={Rs} n={n}: row {i} (slot {slots[i]}) alone")
            check()


# ---- expand ---------------------------------------------------------------------------------------------------------------------------------------------
def _segments(N: int, three: bool):
    if not three:
        return N, N
    return {16: (5, 9), 1000: (600, 800), 4608: (3584, 4096)}[N]


@pytest.fixture(scope="module")
def expand_problems():
    """(N, r) -> T of 16 rows (three r-wide slices), Bt [capacity, r, N] and its chunk-major packing between guards."""
    from vila_amd.lora_serving import pack_b
    cache = {}

    def get(N, r):
        if (N, r) not in cache:
            bt = R.rand_bf16((R.CAPACITY, r, N), 17 + N + r)
            cache[(N, r)] = (R.rand_f32((16, 3 * r), 19 + N + r), bt, R.framed_bank(pack_b(bt)))
        return cache[(N, r)]
    return get


def _expand_call(ops, t16, b_bank, rows, slots, c1, c2, width):
    n = len(rows)
    t = t16[rows][:, :width].clone()
    for i, a in enumerate(slots):
        if a < 0:
            t[i] = float("nan")                                                          # a row without an adapter: its T is not read
    out, check = framed_out_rows(n, b_bank.shape[2], 8, G, dtype=torch.float32)
    ops.lora_expand(framed_operand(t, 8, G), b_bank, R.slots_tensor(slots), out, c1, c2)
    _sync()
    return out, check


@pytest.mark.parametrize("three", [False, True], ids=["one-segment", "qkv-segments"])
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("N", EXPAND_NS)
@pytest.mark.parametrize("n", NS)
def test_expand_every_element(ops, expand_problems, n, N, r, three):
    t16, bt, b_bank = expand_problems(N, r)
    c1, c2 = _segments(N, three)
    width = (3 if three else 1) * r
    rows = list(range(n))
    worst = 0.0
    for kind in R.MAPS:
        slots = R.row_map(kind, n)
        what = f"expand n={n} N={N} r={r} segments={(c1, c2)} [{kind}]"
        out, check = _expand_call(ops, t16, b_bank, rows, slots, c1, c2, width)
        ref, ab = R.expand_ref(t16[:n], bt, slots, c1, c2)
        worst = max(worst, assert_elementwise(out[:n], ref, bgemm_acc_bound(ab, r), what))
        check()
        for i, a in enumerate(slots):
            if a < 0:
                assert R.is_plus_zero(out[i]), f"{what}: row {i} has no adapter and is not +0.0"
        again, _ = _expand_call(ops, t16, b_bank, rows, slots, c1, c2, width)
        assert_bits_equal(again[:n], out[:n], f"{what}: two calls")
    print(f"expand ({n}, {N}, {r}, {three}): worst err / bound {worst:.3f}")


@pytest.mark.parametrize("N,r,three", [(1000, 16, True), (4608, 64, True), (1000, 64, False)])
def test_expand_row_alone_equals_row_of_the_mixed_batch(ops, expand_problems, N, r, three):
    t16, bt, b_bank = expand_problems(N, r)
    c1, c2 = _segments(N, three)
    width = (3 if three else 1) * r
    for n in (9, 16):
        slots = R.row_map("mixed", n)
        out, _ = _expand_call(ops, t16, b_bank, list(range(n)), slots, c1, c2, width)
        for i in range(n):
            solo, check = _expand_call(ops, t16, b_bank, [i], [slots[i]], c1, c2, width)
            assert_bits_equal(solo[0], out[i], f"expand N={N} r={r} n={n}: row {i} (slot {slots[i]}) alone")
            check()


def test_refusals_come_before_any_launch(ops, shrink_problems, expand_problems):
    x16, a_bank = shrink_problems(576, 48)
    out, check = framed_out_rows(0, 48, 8, G, dtype=torch.float32, rows=17)
    x17 = framed_operand(R.rand_bf16((17, 576), 3), 8, G)
    slots17 = R.slots_tensor([0] * 17)
    for n in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            ops.lora_shrink(x17, a_bank, R.scales(), slots17, out, n=n)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.lora_shrink(framed_operand(R.rand_bf16((2, 96), 4), 8, G), R.framed_bank(R.rand_bf16((3, 48, 96), 5)), R.scales(), slots17, out)
    with pytest.raises(ValueError, match="alignment"):
        ops.lora_shrink(framed_operand(R.rand_bf16((2, 576), 6), 4, G), a_bank, R.scales(), slots17, out)
    t16, bt, b_bank = expand_problems(1000, 16)
    outd, checkd = framed_out_rows(0, 1000, 8, G, dtype=torch.float32, rows=17)
    with pytest.raises(ValueError, match="segment ends"):
        ops.lora_expand(framed_operand(t16[:2, :48].clone(), 8, G), b_bank, slots17, outd, 800, 600)
    _sync()
    check(); checkd()


# ---- the addend in the skinny GEMM's epilogue -----------------------------------------------------------------------------------------------------------
class _Problem:
    """16 activation rows, W (and W2), bias, 16 residual rows and 16 addend rows (width N, or 2 N for gate | up), drawn once, with the fp64 products."""
    def __init__(self, N, K, seed, w2=False):
        self.N, self.K = N, K
        self.x16 = R.rand_bf16((16, K), 1000 + seed)
        w = R.rand_bf16((N, K), 2000 + seed, K ** -0.5)
        self.w = framed_operand(w, 0, G)
        self.bias = framed_operand(R.rand_bf16((N,), 3000 + seed), 0, G)
        self.res16 = R.rand_bf16((16, N), 4000 + seed)
        self.d16 = R.rand_f32((16, 2 * N if w2 else N), 6000 + seed, 0.5)
        xd = self.x16.double()
        self.core, self.core_abs = xd @ w.double().t(), xd.abs() @ w.double().abs().t()
        if w2:
            w_up = R.rand_bf16((N, K), 5000 + seed, K ** -0.5)
            self.w2 = framed_operand(w_up, 0, G)
            self.core2, self.core2_abs = xd @ w_up.double().t(), xd.abs() @ w_up.double().abs().t()

    def x(self, n):
        return framed_operand(self.x16[:n], 8, G)

    def addend(self, n, slots):
        """(the framed addend with NaN rows where the row skips it, the fp64 D that the rows which add see: zero elsewhere)"""
        d = self.d16[:n].clone()
        add = torch.tensor([a >= 0 for a in slots], device=d.device)
        d[~add] = float("nan")
        return framed_operand(d, 8, G), torch.where(add[:, None], self.d16[:n].double(), torch.zeros_like(self.d16[:n], dtype=torch.float64))


def _maps(n):
    return [("mixed", R.row_map("mixed", n)), ("one", R.row_map("one", n))]


@pytest.mark.parametrize("n", ADD_NS)
def test_addend_plain_bias_residual_and_fp32_out(ops, n):
    N, K = 40, 576
    prob = _Problem(N, K, seed=n)
    worst = 0.0
    for kind, slots in _maps(n):
        what = f"addend plain n={n} [{kind}]"
        d, d64 = prob.addend(n, slots)
        y, check_y = framed_out_rows(n, N, 8, G)
        f, check_f = framed_out_rows(n, N, 8, G, dtype=torch.float32)
        ops.gemm_batch_lora(prob.x(n), prob.w, d, R.slots_tensor(slots), bias=prob.bias, residual=framed_operand(prob.res16[:n], 8, G), out=y, out_f32=f)
        _sync()
        core, core_abs = prob.core[:n] + d64, prob.core_abs[:n] + d64.abs()
        worst = max(worst, assert_elementwise(y[:n], *bgemm_plain_bound(core, core_abs, K, prob.bias.double(), prob.res16[:n].double()), f"{what} bf16"))
        worst = max(worst, assert_elementwise(f[:n], *bgemm_plain_bound(core, core_abs, K, prob.bias.double(), out_f32=True), f"{what} f32"))
        check_y(); check_f()
    # a NULL addend, and every row -1 (under a NaN addend): the bits of the entry without addend
    y0, _ = framed_out_rows(n, N, 8, G)
    f0, _ = framed_out_rows(n, N, 8, G, dtype=torch.float32)
    res = framed_operand(prob.res16[:n], 8, G)
    ops.gemm_batch(prob.x(n), prob.w, bias=prob.bias, residual=res, out=y0, out_f32=f0)
    for name, d, slots in (("NULL addend", None, None), ("every row -1", prob.addend(n, [-1] * n)[0], R.slots_tensor([-1] * n))):
        y1, check_y = framed_out_rows(n, N, 8, G)
        f1, check_f = framed_out_rows(n, N, 8, G, dtype=torch.float32)
        ops.gemm_batch_lora(prob.x(n), prob.w, d, slots, bias=prob.bias, residual=res, out=y1, out_f32=f1)
        _sync()
        assert_bits_equal(y1[:n], y0[:n], f"plain n={n} {name}: bf16 output vs gemm_batch")
        assert_bits_equal(f1[:n], f0[:n], f"plain n={n} {name}: fp32 output vs gemm_batch")
        check_y(); check_f()
    print(f"addend plain n={n}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("n", ADD_NS)
def test_addend_gateup(ops, n):
    N, K = 40, 576
    prob = _Problem(N, K, seed=100 + n, w2=True)
    worst = 0.0
    for kind, slots in _maps(n):
        d, d64 = prob.addend(n, slots)
        y, check = framed_out_rows(n, N, 8, G)
        ops.gemm_batch_lora(prob.x(n), prob.w, d, R.slots_tensor(slots), w2=prob.w2, out=y)
        _sync()
        dg, du = d64[:, :N], d64[:, N:]
        ref, bound = bgemm_gateup_bound(prob.core[:n] + dg, prob.core_abs[:n] + dg.abs(), prob.core2[:n] + du, prob.core2_abs[:n] + du.abs(), K)
        worst = max(worst, assert_elementwise(y[:n], ref, bound, f"addend gate/up n={n} [{kind}]"))
        check()
    y0, _ = framed_out_rows(n, N, 8, G)
    ops.gemm_batch(prob.x(n), prob.w, w2=prob.w2, out=y0)
    for name, d, slots in (("NULL addend", None, None), ("every row -1", prob.addend(n, [-1] * n)[0], R.slots_tensor([-1] * n))):
        y1, check = framed_out_rows(n, N, 8, G)
        ops.gemm_batch_lora(prob.x(n), prob.w, d, slots, w2=prob.w2, out=y1)
        _sync()
        assert_bits_equal(y1[:n], y0[:n], f"gate/up n={n} {name}: vs gemm_batch")
        check()
    print(f"addend gate/up n={n}: worst err / bound {worst:.3f}")


def _qkv_call(ops, prob, heads, n, cs16, d, slots, lora=True):
    nq, nkv, hd = heads
    q, check_q = framed_out_rows(n, nq * hd, 8, G)
    kc, check_k = framed_cache(nkv, MAX_CTX, hd)
    vc, check_v = framed_cache(nkv, MAX_CTX, hd)
    pos = list(POS16[:n])
    pos_t = framed_operand(torch.tensor(pos, dtype=torch.int32, device="cuda"), 0, 1, pad=MAX_CTX - 1)
    cs = framed_operand(cs16[:n].reshape(-1), 0, G).view(n, hd)
    if lora:
        ops.qkv_batch_lora(prob.x(n), prob.w, prob.bias, q, kc, vc, pos_t, cs, nq, nkv, hd, d, slots)
    else:
        ops.qkv_batch(prob.x(n), prob.w, prob.bias, q, kc, vc, pos_t, cs, nq, nkv, hd)
    _sync()
    return q, kc, vc, pos, (check_q, check_k, check_v)


@pytest.mark.parametrize("n", ADD_NS)
def test_addend_qkv_in_front_of_rope_and_the_cache_append(ops, n):
    heads, K = (3, 1, 64), 576
    nq, nkv, hd = heads
    N = (nq + 2 * nkv) * hd
    prob = _Problem(N, K, seed=200 + n)
    cs16 = rope_table(ROPE_POS16, hd, device="cuda")
    worst = 0.0
    for kind, slots in _maps(n):
        d, d64 = prob.addend(n, slots)
        q, kc, vc, pos, checks = _qkv_call(ops, prob, heads, n, cs16, d, R.slots_tensor(slots))
        ref, bound = bgemm_qkv_bound(prob.core[:n] + d64, prob.core_abs[:n] + d64.abs(), K, prob.bias.double(), cs16[:n].double(), nq, nkv, hd)
        worst = max(worst, assert_qkv_outputs(q, kc, vc, checks, pos, n, ref, bound, nq, nkv, hd, f"addend qkv n={n} [{kind}]"))
    q0, kc0, vc0, _, _ = _qkv_call(ops, prob, heads, n, cs16, None, None, lora=False)
    for name, d, slots in (("NULL addend", None, None), ("every row -1", prob.addend(n, [-1] * n)[0], R.slots_tensor([-1] * n))):
        q1, kc1, vc1, pos, checks = _qkv_call(ops, prob, heads, n, cs16, d, slots)
        assert_bits_equal(q1[:n], q0[:n], f"qkv n={n} {name}: q vs qkv_batch")
        assert_bits_equal(kc1, kc0, f"qkv n={n} {name}: K cache vs qkv_batch")
        assert_bits_equal(vc1, vc0, f"qkv n={n} {name}: V cache vs qkv_batch")
        checks[0](); checks[1](pos, n); checks[2](pos, n)
    print(f"addend qkv n={n}: worst err / bound {worst:.3f}")

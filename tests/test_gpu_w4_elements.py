"""Every element of the three W4A16 kernels, in framed buffers: gemv_w4.hip (solo decode), gemv_w4_batch.hip (batched decode), gemm_w4.hip (prefill).

The other W4 files judge a whole vector or matrix by one rel-L2 figure (1e-2; 1.5e-2 gate/up; 3e-2 on the logits of a model), inside which a wrong
zero point of one group, a wave seam off by one group, a swapped nibble pair or a dropped K slab of one tile all fit (tests/test_w4_bound_cpu.py
shows which).  The two fused q|k|v kernels had no operator test at all; they run here through vila_qkv_w4_bf16 / vila_qkv_w4_batch_bf16.

Every case runs in two regimes (tests/gpu_util.py, proved on the CPU by tests/test_w4_bound_cpu.py):
  exact    integer activations |x| <= 4 and exact_w4 weights with power-of-two scales (w4_exact_case): every partial sum of the kernels is an
           integer multiple of 2^kmin below 2^24 of them, so the fp32 value before the epilogue is the fp64 product whatever the order of groups,
           waves, tiles, K slices or ring depths.  Plain outputs (modes 0, the V heads, the prefill's q|k|v form) must equal w4_exact_plain_ref BIT FOR
           BIT.  Gate/up and the RoPE'd q and k heads stay inside bgemm_gateup_bound / bgemm_qkv_bound with the accumulation term set to ZERO: only
           the epilogue's own roundings and silu_f's error remain.  The fused RMSNorm of the solo kernel stays exact with |x_k| = 2 and integer
           gains (w4_exact_case's docstring).
  generic  Gaussian activations, AWQ-quantised Gaussian weights (bf16 scales that are no powers of two): |out - ref64| <= w4_generic_bound at every
           element, ref64 the product with the dequantised weights.
Buffers as in tests/test_gpu_batch_gemm_elements.py: x, norm_w, bias and residual are views with NaN around them (batched x: ldx = K + 8), outputs
are views of buffers that hold a bit pattern and everything outside the view must still hold it, the KV caches are [slots][kv][8][head_dim] of the
pattern between guard slots where only (slot m, every kv head, pos[m]) with pos[m] < 8 may change, the prefill's workspace has exactly
vila_gemm_w4_workspace_bytes between two guards.  Every case runs twice and must give the same bits; a device fault ends the session (_sync).

Shapes, the smallest at which each mechanism engages.
  solo     K: 128 (one group, one wave), 896 (one full batch of UB = 7), 1024 (two waves), 1920 (three waves of 5), 14336 (16 waves x 7), 14464 (the
           first "deep" shape, UB = 10), 20608 (more than 10 groups per wave: a second batch inside a tile), 24704 (stage_x_w4 leaves its register
           path); N in {2, 5, 16, 37}; (8208, 13568) and gate/up (4100, 13568): 513 tiles on 256 persistent blocks, block 0 walks three and
           reuses both parity buffers; (16, 32768): 67 KB of LDS, above the 64 KB a kernel gets unasked.  q|k|v heads (2, 1, 16), (2, 1, 32),
           (3, 1, 64), (28, 4, 128) at positions 3, 7 = max_ctx - 1, 8 = max_ctx and 13 (the last two write q and no K/V).
  batched  n in {1, 4, 5, 8, 9, 16}; 511 / 512 / 513 / 1023 / 1024 / 1025 tiles at K = 128 .. 384 (T = 1 -> 2 -> 4; at 513 and 1025 the last item is
           part-filled); (16384, 18944): T = 4, W capped at 8, UB = 2, ten batches per wave; (4112, 13568): 257 items on 256 blocks at T = 1;
           (16400, 6400): 257 items on 256 blocks at T = 4; the q|k|v heads above with POS16 / ROPE_POS16; row m of an n-row call is bit-equal to the
           row alone and to row m of the 16-row call.
  prefill  M in {1, 63, 64, 65, 129} x N in {16, 144 (the last block holds one live tile of eight), 2048} x K in {128 (splits clamped to G = 1), 384
           (3 = G), 2560 (8 uneven slices of 20 groups)}, K rotating; (1024, 2048, 256): 256 blocks, un-sliced; q|k|v heads of 32 / 64 / 128.
  cross    exact regime: the solo GEMV, row m of the batched GEMV and row m of the prefill GEMM give the same bits on one matrix, modes 0 and 1.

Measured on an MI355X (every test prints its figure with -s), generic regime, worst err / bound over all cases of a kernel and mode:
    solo     plain 0.74   gate/up 0.69   q|k|v 0.996
    batched  plain 0.88   gate/up 0.87   q|k|v 0.996
    prefill  plain 0.86   gate/up 0.87   q|k|v (natural order, no RoPE) 0.79
The figures near 1 are the last bf16 rounding alone (an element at the bottom of its binade, half a spacing off); where the accumulation term
dominates a correct kernel uses a fifth to a third of the bound: 0.20 at solo (8208, 13568), 0.24 at batched (16, 16384, 18944), 0.33 at batched
(16, 16400, 6400).  Every exact-regime plain element was bit-equal; no kernel fault was found.  The whole file (150 tests) takes 7 s."""
import functools
import itertools

import pytest
import torch

from tests.gpu_util import (assert_bits_equal, assert_elementwise, assert_qkv_outputs, cache_rows, framed_cache, framed_flat, framed_operand, framed_out,
                            framed_out_rows, framed_ws, rope_table, w4_exact_case, w4_exact_plain_ref, w4_generic_acc, w4_generic_bound, w4_staged_norm,
                            w4_unpack)
from tests.test_gpu_batch_gemm_elements import MAX_CTX, NS_ROWS, POS16, ROPE_POS16, _bits, _sync

pytestmark = pytest.mark.gpu

G = 4                                                    # guard rows / slots around every framed operand and output
REGIMES = ("exact", "generic")
SCALE_SETS = ((-7, -6, -5), (-9, -8, -7))                # the exact regime's log2 scales: a case takes SCALE_SETS[seed % 2]
X_MAX = 4
EPS = 1e-6
HEADS = ((2, 1, 16), (2, 1, 32), (3, 1, 64), (28, 4, 128))

SOLO_KS = (128, 896, 1024, 1920, 14336, 14464, 20608, 24704)
SOLO_NS = (2, 5, 16, 37)
SOLO_SHAPES = [(SOLO_NS[(i + j) % 4], K) for j in (0, 2) for i, K in enumerate(SOLO_KS)]
SOLO_PIPE, SOLO_PIPE_GATEUP, SOLO_LDS = (8208, 13568), (4100, 13568), (16, 32768)
SOLO_POS = (3, MAX_CTX - 1, MAX_CTX, MAX_CTX + 5)
SOLO_QKV_KS = (128, 1024, 1920, 3584)
SOLO_QKV = [(h, SOLO_QKV_KS[(i + j) % 4], p) for (i, h), (j, p) in itertools.product(enumerate(HEADS), enumerate(SOLO_POS))]

BATCH_SMALL = [(n, (4, 20, 37)[(i + j) % 3], (128, 896, 1024)[j]) for (i, n), j in itertools.product(enumerate(NS_ROWS), range(3)) if (i + j) % 2 == 0]
BATCH_TILES = [(NS_ROWS[i], t, (128, 256, 384)[i % 3]) for i, t in enumerate((511, 512, 513, 1023, 1024, 1025))]      # (n, tiles, K)
BATCH_WALK = [(9, 257, 13568), (16, 1025, 6400)]         # (n, tiles, K): 257 items on 256 resident blocks at T = 1 and at T = 4
BATCH_DEEP = (16, 1024, 18944)
BATCH_QKV_KS = (128, 384, 1152)
BATCH_QKV = [(h, n, BATCH_QKV_KS[(i + j) % 3], bool((i + j) % 2)) for (i, h), (j, n) in itertools.product(enumerate(HEADS), enumerate(NS_ROWS))]

PREFILL_MS, PREFILL_NS, PREFILL_KS = (1, 63, 64, 65, 129), (16, 144, 2048), (128, 384, 2560)
PREFILL_SHAPES = [(M, N, PREFILL_KS[(i + j) % 3]) for (i, M), (j, N) in itertools.product(enumerate(PREFILL_MS), enumerate(PREFILL_NS))] + [(1024, 2048, 256)]
PREFILL_QKV = [(h, PREFILL_MS[(i + 1) % 5], PREFILL_KS[i % 3]) for i, h in enumerate(HEADS[1:])]


def _rows_of_tiles(tiles: int, part: bool, gateup: bool) -> int:
    """N of a matrix of `tiles` 16-row tiles, the last one half filled where `part`."""
    rows = tiles * 16 - (8 if part else 0)
    return rows // 2 if gateup else rows


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib, ops as _ops
    _lib.load()
    return _ops


class _Prob:
    """One matrix with `rows` activation rows, bias and residual rows, in one regime; core / acc (and core_up / acc_up) [rows, N] fp64 are the
    reference product and the accumulation term of the bound (zero in the exact regime), computed once."""
    def __init__(self, regime, N, K, seed, gateup=False, heads=None, normed=False, rows=16):
        from vila_amd.quant import W4Matrix, rope_interleave_rows
        self.exact, self.N, self.K, self.gateup, self.heads, self.normed = regime == "exact", N, K, gateup, heads, normed
        if self.exact:
            c = w4_exact_case(N, K, seed, SCALE_SETS[seed % 2], X_MAX, rows, gateup, heads, normed, device="cuda")
            self.mat, self.x, self.norm_w, self.bias, self.res = c["mat"], c["x"], c["norm_w"], c["bias"], c["res"]
            self.core, self.core_up = c["core"], c.get("core_up")
            self.acc = torch.zeros_like(self.core)
            self.acc_up = self.acc
            return
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *shape: torch.randn(shape, generator=g, device="cuda")
        perm = rope_interleave_rows(heads[0] + heads[1], heads[0] + 2 * heads[1], heads[2], device="cuda") if heads is not None else None
        self.mat = W4Matrix.pack(rnd(N, K) * 0.03, rnd(N, K) * 0.03 if gateup else None, row_perm=perm)
        self.x = rnd(rows, K).to(torch.bfloat16)
        self.bias, self.res = rnd(N).to(torch.bfloat16), rnd(rows, N).to(torch.bfloat16)
        x_eff, slack, self.norm_w = self.x.double(), None, None
        if normed:
            self.norm_w = (1.0 + 0.1 * rnd(K)).to(torch.bfloat16)
            staged, slack = w4_staged_norm(self.x.double(), self.norm_w.double(), EPS)
            x_eff = staged.double()
        q, z, s = w4_unpack(self.mat.logical)
        if gateup:
            self.core, self.acc = w4_generic_acc(x_eff, q[0::2], z[0::2], s[0::2], slack)
            self.core_up, self.acc_up = w4_generic_acc(x_eff, q[1::2], z[1::2], s[1::2], slack)
        else:
            self.core, self.acc = w4_generic_acc(x_eff, q, z, s, slack)
            self.core_up = self.acc_up = None

    def check_plain(self, out, rows, use_bias, use_res, what):
        """out [r, N] bf16 against rows `rows` of the problem -> err / bound (0 in the exact regime, where the bits must match)."""
        b, r = self.bias.double() if use_bias else None, self.res[rows].double() if use_res else None
        if self.exact:
            assert_bits_equal(out, w4_exact_plain_ref(self.core[rows], b, r), what)
            return 0.0
        return assert_elementwise(out, *w4_generic_bound("plain", self.K, self.core[rows], self.acc[rows], bias64=b, res64=r), what)

    def check_gateup(self, out, rows, what):
        return assert_elementwise(out, *w4_generic_bound("gateup", self.K, self.core[rows], self.acc[rows], self.core_up[rows], self.acc_up[rows]), what)

    def check_qkv(self, q, kc, vc, checks, pos, rows, use_bias, cs, what):
        """q [>= r, q * hd], caches [slots, kv, ctx, hd]; the V rows of the exact regime bit for bit as well."""
        nq, nkv, hd = self.heads
        n = self.core[rows].shape[0]
        b = self.bias.double() if use_bias else None
        ref, bound = w4_generic_bound("qkv", self.K, self.core[rows], self.acc[rows], bias64=b, cs64=cs.double(), heads=self.heads)
        worst = assert_qkv_outputs(q, kc, vc, checks, pos, n, ref, bound, nq, nkv, hd, what)
        if self.exact:
            got, live = cache_rows(vc, pos, n)
            if live:
                v0 = (nq + nkv) * hd
                want = w4_exact_plain_ref(self.core[rows][live, v0:], None if b is None else b[v0:])
                assert_bits_equal(got, want, f"{what} V rows of {live}")
        return worst


@functools.lru_cache(maxsize=2)
def _prob(regime, N, K, seed, gateup=False, heads=None, normed=False, rows=16):
    return _Prob(regime, N, K, seed, gateup, heads, normed, rows)


def _report(what, worst):
    print(f"W4 {what}: generic worst err / bound {worst:.3f}")


# ---- solo: gemv_w4_kernel<0 / 1 / 3> ----------------------------------------------------------------------------------------------------------------------
def _solo_call(ops, p, m, use_bias=False, use_res=False):
    y, check = framed_flat(p.N)
    ops.gemv_w4(framed_operand(p.x[m], 0, 1), p.mat, norm_w=framed_operand(p.norm_w, 0, 1) if p.normed else None, eps=EPS,
                bias=framed_operand(p.bias, 0, 1) if use_bias else None, residual=framed_operand(p.res[m], 0, 1) if use_res else None, out=y)
    _sync()
    return y, check


def _solo_plain(ops, N, K, what, rows=2, epilogues=((False, False), (True, False), (False, True), (True, True))):
    worst = 0.0
    for regime, normed in itertools.product(REGIMES, (False, True)):
        p = _prob(regime, N, K, N + K, normed=normed, rows=rows)
        for (use_bias, use_res), m in itertools.product(epilogues, range(rows)):
            w = f"{what} {regime} norm={normed} bias={use_bias} residual={use_res} row {m}"
            y, check = _solo_call(ops, p, m, use_bias, use_res)
            worst = max(worst, p.check_plain(y[None], slice(m, m + 1), use_bias, use_res, w))
            check()
            assert torch.equal(_bits(y), _bits(_solo_call(ops, p, m, use_bias, use_res)[0])), f"{w}: two calls differ"
    _report(what, worst)


def _solo_gateup(ops, N, K, what, rows=2):
    worst = 0.0
    for regime, normed in itertools.product(REGIMES, (False, True)):
        p = _prob(regime, N, K, N + K + 1, gateup=True, normed=normed, rows=rows)
        for m in range(rows):
            w = f"{what} {regime} norm={normed} row {m}"
            y, check = _solo_call(ops, p, m)
            worst = max(worst, p.check_gateup(y[None], slice(m, m + 1), w))
            check()
            assert torch.equal(_bits(y), _bits(_solo_call(ops, p, m)[0])), f"{w}: two calls differ"
    _report(what, worst)


@pytest.mark.parametrize("N,K", SOLO_SHAPES, ids=str)
def test_solo_plain(ops, N, K):
    _solo_plain(ops, N, K, f"solo plain ({N}, {K})")


@pytest.mark.parametrize("N,K", SOLO_SHAPES, ids=str)
def test_solo_gateup(ops, N, K):
    _solo_gateup(ops, N, K, f"solo gate/up ({N}, {K})")


def test_solo_plain_persistent_blocks(ops):
    """513 tiles on 256 resident blocks of 16 waves (gemv_w4.hip:299-301): gemv_w4_kernel<0, 7, true>, block 0 walks tiles 0, 256 and 512."""
    _solo_plain(ops, *SOLO_PIPE, f"solo plain {SOLO_PIPE} PIPE", rows=1, epilogues=((False, False), (True, True)))


def test_solo_gateup_persistent_blocks(ops):
    """2 N = 8200 packed rows: 513 tiles, the last one half filled; gemv_w4_kernel<1, 7, true>."""
    _solo_gateup(ops, *SOLO_PIPE_GATEUP, f"solo gate/up {SOLO_PIPE_GATEUP} PIPE", rows=1)


def test_solo_lds_above_64k(ops):
    """K = 32768 needs 68672 bytes of LDS.  launch_gemv_w4 admits up to 160 KB, what a CU has, and raises the instantiation's dynamic-LDS limit
    before the first such launch (gemv_w4.hip W4_LAUNCH), as its batched sibling does: the result is exact, not a failed launch."""
    N, K = SOLO_LDS
    p = _prob("exact", N, K, N + K, rows=1)
    for use_bias, use_res in ((False, False), (True, True)):
        y, check = _solo_call(ops, p, 0, use_bias, use_res)
        p.check_plain(y[None], slice(0, 1), use_bias, use_res, f"solo plain ({N}, {K}) bias={use_bias} residual={use_res}")
        check()
        assert torch.equal(_bits(y), _bits(_solo_call(ops, p, 0, use_bias, use_res)[0]))


def _solo_qkv_call(ops, p, m, pos, use_bias, cs):
    nq, nkv, hd = p.heads
    q, check_q = framed_flat(nq * hd)
    kc, check_k = framed_cache(nkv, MAX_CTX, hd, slots=1)
    vc, check_v = framed_cache(nkv, MAX_CTX, hd, slots=1)
    pos_t = framed_operand(torch.tensor([pos], dtype=torch.int32, device="cuda"), 0, 1, pad=MAX_CTX - 1)
    ops.qkv_w4(framed_operand(p.x[m], 0, 1), p.mat, framed_operand(p.bias, 0, 1) if use_bias else None, q, kc[0], vc[0], pos_t, framed_operand(cs, 0, 1),
               nq, nkv, hd, norm_w=framed_operand(p.norm_w, 0, 1) if p.normed else None, eps=EPS)
    _sync()
    return q, kc, vc, (check_q, check_k, check_v)


@pytest.mark.parametrize("heads,K,pos", SOLO_QKV, ids=str)
def test_solo_qkv_rope_and_cache_rows(ops, heads, K, pos):
    nq, nkv, hd = heads
    N = (nq + 2 * nkv) * hd
    cs = rope_table([ROPE_POS16[pos]], hd, device="cuda")
    worst = 0.0
    for regime, normed, use_bias in itertools.product(REGIMES, (False, True), (False, True)):
        p = _prob(regime, N, K, N + K + 2, heads=heads, normed=normed, rows=1)
        what = f"solo qkv {heads} K={K} pos={pos} {regime} norm={normed} bias={use_bias}"
        q, kc, vc, checks = _solo_qkv_call(ops, p, 0, pos, use_bias, cs[0])
        worst = max(worst, p.check_qkv(q[None], kc, vc, checks, [pos], slice(0, 1), use_bias, cs, what))
        q2, kc2, vc2, _ = _solo_qkv_call(ops, p, 0, pos, use_bias, cs[0])
        assert torch.equal(_bits(q), _bits(q2)) and torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2)), f"{what}: two calls differ"
    _report(f"solo qkv {heads} K={K} pos={pos}", worst)


# ---- batched: gemv_w4_batch_kernel<0 / 1 / 2, T, UB> --------------------------------------------------------------------------------------------------------
def _batch_call(ops, p, rows, use_bias=False, use_res=False, inplace=False):
    n = len(range(*rows.indices(16)))
    out, check = framed_out_rows(n, p.N, 0, G, fill=p.res[rows] if inplace else None)
    res = out if inplace else (framed_operand(p.res[rows], 0, G) if use_res else None)
    ops.gemv_w4_batch(framed_operand(p.x[rows], 8, G), p.mat, bias=framed_operand(p.bias, 0, G) if use_bias else None, residual=res, out=out, n=n)
    _sync()
    return out, check


def _batch_case(ops, n, N, K, gateup, what, solo_rows=None, epilogues=((False, False, False), (True, True, False), (True, True, True))):
    """One (n, N, K) in both regimes: every element, the frame, two calls, the rows of the 16-row call, the rows alone (`solo_rows`: all by default)."""
    worst = 0.0
    for regime in REGIMES:
        p = _prob(regime, N, K, n + N + K, gateup=gateup)
        for use_bias, use_res, inplace in ((False, False, False),) if gateup else epilogues:
            w = f"{what} {regime} bias={use_bias} residual={use_res} inplace={inplace}"
            kw = dict(use_bias=use_bias, use_res=use_res, inplace=inplace)
            out, check = _batch_call(ops, p, slice(0, n), **kw)
            worst = max(worst, p.check_gateup(out[:n], slice(0, n), w) if gateup else p.check_plain(out[:n], slice(0, n), use_bias, use_res, w))
            check()
            assert torch.equal(_bits(out[:n]), _bits(_batch_call(ops, p, slice(0, n), **kw)[0][:n])), f"{w}: two calls differ"
            full, check16 = _batch_call(ops, p, slice(0, 16), **kw)
            assert torch.equal(_bits(out[:n]), _bits(full[:n])), f"{w}: rows differ from those of the 16-row call"
            check16()
            for m in range(n) if solo_rows is None else solo_rows:
                one, check1 = _batch_call(ops, p, slice(m, m + 1), **kw)
                assert torch.equal(_bits(out[m]), _bits(one[0])), f"{w}: row {m} differs from the row computed alone"
                check1()
    _report(what, worst)


@pytest.mark.parametrize("gateup", [False, True], ids=["plain", "gateup"])
@pytest.mark.parametrize("n,N,K", BATCH_SMALL, ids=str)
def test_batch_small(ops, n, N, K, gateup):
    _batch_case(ops, n, N, K, gateup, f"batch {'gate/up' if gateup else 'plain'} ({n}, {N}, {K})")


@pytest.mark.parametrize("gateup", [False, True], ids=["plain", "gateup"])
@pytest.mark.parametrize("n,tiles,K", BATCH_TILES, ids=str)
def test_batch_tile_count_switch(ops, n, tiles, K, gateup):
    """launch_gemv_w4_batch:201: T = 1 below 512 tiles, 2 from 512, 4 from 1024; at 513 and 1025 tiles the last item holds one tile, half filled."""
    N = _rows_of_tiles(tiles, tiles in (513, 1025), gateup)
    _batch_case(ops, n, N, K, gateup, f"batch {'gate/up' if gateup else 'plain'} ({n}, {N}, {K}) {tiles} tiles", solo_rows=(0, n - 1))


@pytest.mark.parametrize("gateup", [False, True], ids=["plain", "gateup"])
@pytest.mark.parametrize("n,tiles,K", BATCH_WALK, ids=str)
def test_batch_persistent_blocks(ops, n, tiles, K, gateup):
    """257 items on 256 resident blocks (launch_w4b_t:172-173): block 0 walks items 0 and 256, the second part-filled, on the other parity buffer."""
    N = _rows_of_tiles(tiles, False, gateup)
    _batch_case(ops, n, N, K, gateup, f"batch {'gate/up' if gateup else 'plain'} ({n}, {N}, {K}) walking", solo_rows=(n - 1,), epilogues=((True, True, False),))


def test_batch_deep_k_at_four_tiles(ops):
    """K = 18944 at T = 4: W is capped at 8 waves of 18-19 groups, UB = 2: ten load batches per wave and item."""
    n, tiles, K = BATCH_DEEP
    _batch_case(ops, n, tiles * 16, K, False, f"batch plain ({n}, {tiles * 16}, {K}) T=4", solo_rows=(5,), epilogues=((True, True, False),))


def _batch_qkv_call(ops, p, rows, use_bias, cs16):
    nq, nkv, hd = p.heads
    idx = list(range(*rows.indices(16)))
    n = len(idx)
    q, check_q = framed_out_rows(n, nq * hd, 8, G)
    kc, check_k = framed_cache(nkv, MAX_CTX, hd)
    vc, check_v = framed_cache(nkv, MAX_CTX, hd)
    pos = [POS16[m] for m in idx]
    pos_t = framed_operand(torch.tensor(pos, dtype=torch.int32, device="cuda"), 0, 1, pad=MAX_CTX - 1)
    cs = framed_operand(cs16[rows].reshape(-1), 0, G).view(n, hd)
    ops.qkv_w4_batch(framed_operand(p.x[rows], 8, G), p.mat, framed_operand(p.bias, 0, G) if use_bias else None, q, kc, vc, pos_t, cs, nq, nkv, hd)
    _sync()
    return q, kc, vc, pos, (check_q, check_k, check_v)


@pytest.mark.parametrize("heads,n,K,use_bias", BATCH_QKV, ids=str)
def test_batch_qkv_rope_and_cache_rows(ops, heads, n, K, use_bias):
    nq, nkv, hd = heads
    N = (nq + 2 * nkv) * hd
    cs16 = rope_table(ROPE_POS16, hd, device="cuda")
    worst = 0.0
    for regime in REGIMES:
        p = _prob(regime, N, K, n + N + K + 2, heads=heads)
        what = f"batch qkv {heads} n={n} K={K} bias={use_bias} {regime}"
        rows = slice(0, n)
        q, kc, vc, pos, checks = _batch_qkv_call(ops, p, rows, use_bias, cs16)
        worst = max(worst, p.check_qkv(q, kc, vc, checks, pos, rows, use_bias, cs16[:n], what))
        q2, kc2, vc2, _, _ = _batch_qkv_call(ops, p, rows, use_bias, cs16)
        assert torch.equal(_bits(q[:n]), _bits(q2[:n])) and torch.equal(_bits(kc), _bits(kc2)) and torch.equal(_bits(vc), _bits(vc2)), f"{what}: two calls differ"
        qf, kcf, vcf, _, checks16 = _batch_qkv_call(ops, p, slice(0, 16), use_bias, cs16)
        assert torch.equal(_bits(q[:n]), _bits(qf[:n])) and torch.equal(_bits(kc[:n]), _bits(kcf[:n])) and torch.equal(_bits(vc[:n]), _bits(vcf[:n])), \
            f"{what}: rows differ from those of the 16-row call"
        checks16[0](); checks16[1](POS16, 16); checks16[2](POS16, 16)
        for m in range(n):
            q1, kc1, vc1, _, checks1 = _batch_qkv_call(ops, p, slice(m, m + 1), use_bias, cs16)
            assert torch.equal(_bits(q[m]), _bits(q1[0])) and torch.equal(_bits(kc[m]), _bits(kc1[0])) and torch.equal(_bits(vc[m]), _bits(vc1[0])), \
                f"{what}: row {m} differs from the row computed alone"
            checks1[0](); checks1[1](POS16[m:m + 1], 1); checks1[2](POS16[m:m + 1], 1)
    _report(f"batch qkv {heads} n={n} K={K} bias={use_bias}", worst)


# ---- prefill: gemm_w4_kernel (+ gemm_w4_reduce_kernel) ------------------------------------------------------------------------------------------------------
def _prefill_call(ops, p, M, use_bias=False, use_res=False, heads=None):
    from vila_amd import _lib
    out, check = framed_out(M, p.N, 0, G)
    ws, check_ws = framed_ws(int(_lib.load().vila_gemm_w4_workspace_bytes(M, p.N, p.K, 2 if heads is not None else p.mat.mode)))
    ops.gemm_w4(framed_operand(p.x[:M], 0, G), p.mat, bias=framed_operand(p.bias, 0, G) if use_bias else None,
                residual=framed_operand(p.res[:M], 0, G) if use_res else None, out=out, heads=heads, ws=ws)
    _sync()
    return out, lambda: (check(), check_ws())


@pytest.mark.parametrize("gateup", [False, True], ids=["plain", "gateup"])
@pytest.mark.parametrize("M,N,K", PREFILL_SHAPES, ids=str)
def test_prefill(ops, M, N, K, gateup):
    what = f"prefill {'gate/up' if gateup else 'plain'} ({M}, {N}, {K})"
    worst = 0.0
    for regime in REGIMES:
        p = _prob(regime, N, K, M + N + K, gateup=gateup, rows=M)
        for use_bias, use_res in ((False, False),) if gateup else ((False, False), (True, False), (True, True)):
            w = f"{what} {regime} bias={use_bias} residual={use_res}"
            out, check = _prefill_call(ops, p, M, use_bias, use_res)
            worst = max(worst, p.check_gateup(out, slice(0, M), w) if gateup else p.check_plain(out, slice(0, M), use_bias, use_res, w))
            check()
            assert torch.equal(_bits(out), _bits(_prefill_call(ops, p, M, use_bias, use_res)[0])), f"{w}: two calls differ"
    _report(what, worst)


@pytest.mark.parametrize("heads,M,K", PREFILL_QKV, ids=str)
def test_prefill_qkv_natural_order(ops, heads, M, K):
    """Mode 2 (gemm_w4.hip:56-64): the RoPE-interleaved packed rows of the q and k heads come back in natural column order with the bias added and
    nothing else, a plain epilogue: bit-equal in the exact regime."""
    nq, nkv, hd = heads
    N = (nq + 2 * nkv) * hd
    what = f"prefill qkv {heads} M={M} K={K}"
    worst = 0.0
    for regime, use_bias in itertools.product(REGIMES, (False, True)):
        p = _prob(regime, N, K, M + N + K + 2, heads=heads, rows=M)
        w = f"{what} {regime} bias={use_bias}"
        out, check = _prefill_call(ops, p, M, use_bias, heads=heads)
        worst = max(worst, p.check_plain(out, slice(0, M), use_bias, False, w))
        check()
        assert torch.equal(_bits(out), _bits(_prefill_call(ops, p, M, use_bias, heads=heads)[0])), f"{w}: two calls differ"
    _report(what, worst)


# ---- the three kernels on one matrix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gateup", [False, True], ids=["plain", "gateup"])
@pytest.mark.parametrize("N,K", [(48, 1920), (16, 14464)], ids=str)
def test_three_kernels_same_bits(ops, N, K, gateup):
    """Exact regime: the fp32 value before the epilogue is the same in all three kernels, and their epilogues round alike (gemv_w4.hip:231-238,
    gemv_w4_batch.hip:116-123, gemm_w4.hip:54-69): the solo GEMV of row m, row m of the batched GEMV and row m of the prefill GEMM are bit-equal."""
    p = _prob("exact", N, K, N + K + 7, gateup=gateup)
    for use_bias, use_res in ((False, False),) if gateup else ((False, False), (True, True)):
        what = f"three kernels ({N}, {K}) gateup={gateup} bias={use_bias} residual={use_res}"
        batch, _ = _batch_call(ops, p, slice(0, 16), use_bias, use_res)
        prefill, _ = _prefill_call(ops, p, 16, use_bias, use_res)
        assert torch.equal(_bits(batch), _bits(prefill)), f"{what}: the batched GEMV and the prefill GEMM differ at (row, col) {(_bits(batch) != _bits(prefill)).nonzero()[:8].tolist()}"
        for m in range(16):
            solo, _ = _solo_call(ops, p, m, use_bias, use_res)
            assert torch.equal(_bits(solo), _bits(batch[m])), f"{what}: the solo GEMV of row {m} differs at columns {(_bits(solo) != _bits(batch[m])).nonzero()[:8].flatten().tolist()}"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def test_qkv_entries_refuse_before_any_launch(ops):
    """NULL pointers, head_dim 24, K = 192, n = 0 and 17, a q row stride shorter than its row: -1 with a message, nothing written, and a correct
    call afterwards still passes."""
    from vila_amd import _lib
    lib = _lib.load()
    heads, K = (2, 1, 16), 128
    nq, nkv, hd = heads
    p = _prob("exact", 64, K, 9, heads=heads)
    s = torch.cuda.current_stream().cuda_stream
    q, check_q = framed_out_rows(0, nq * hd, 8, G)
    kc, check_k = framed_cache(nkv, MAX_CTX, hd)
    vc, check_v = framed_cache(nkv, MAX_CTX, hd)
    pos = torch.zeros(16, dtype=torch.int32, device="cuda")
    cs = rope_table(ROPE_POS16, hd, device="cuda")
    x = framed_operand(p.x[:2], 8, G)
    mq, msz = p.mat.q.data_ptr(), p.mat.sz.data_ptr()
    solo = lambda **kw: lib.vila_qkv_w4_bf16(*[kw.get(k, v) for k, v in (("x", x.data_ptr()), ("norm_w", None), ("eps", 0.0), ("Wq", mq), ("Wsz", msz), ("bias", None),
                                                                              ("q", q.data_ptr()), ("k", kc.data_ptr()), ("v", vc.data_ptr()), ("pos", pos.data_ptr()),
                                                                              ("cs", cs.data_ptr()), ("nq", nq), ("nkv", nkv), ("hd", hd), ("ctx", MAX_CTX), ("K", K))], s)
    batch = lambda **kw: lib.vila_qkv_w4_batch_bf16(*[kw.get(k, v) for k, v in (("x", x.data_ptr()), ("ldx", x.stride(0)), ("n", 2), ("Wq", mq), ("Wsz", msz), ("bias", None),
                                                                                     ("q", q.data_ptr()), ("ldq", q.stride(0)), ("k", kc.data_ptr()), ("v", vc.data_ptr()),
                                                                                     ("slot", kc.stride(0)), ("pos", pos.data_ptr()), ("cs", cs.data_ptr()), ("nq", nq),
                                                                                     ("nkv", nkv), ("hd", hd), ("ctx", MAX_CTX), ("K", K))], s)
    for call, kw, pat in ((solo, {"q": None}, "NULL"), (solo, {"pos": None}, "NULL"), (solo, {"hd": 24}, "head_dim"), (solo, {"K": 192}, "multiple of the 128"),
                          (solo, {"ctx": 0}, "max_ctx"), (batch, {"Wsz": None}, "NULL"), (batch, {"n": 0}, "1..16"), (batch, {"n": 17}, "1..16"),
                          (batch, {"K": 192, "ldx": 192}, "multiple of the 128"), (batch, {"hd": 24}, "head_dim"), (batch, {"ldq": nq * hd - 8}, "row stride")):
        assert call(**kw) == -1, (kw, pat)
        assert pat in lib.vila_last_error().decode(), (kw, lib.vila_last_error().decode())
    with pytest.raises(ValueError, match="q.k.v rows"):
        ops.qkv_w4_batch(x, p.mat, None, q, kc, vc, pos, cs, 3, 1, 16)
    _sync()
    check_q(); check_k([], 0); check_v([], 0)
    cs16 = rope_table(ROPE_POS16, hd, device="cuda")
    qq, kk, vv, pp, checks = _batch_qkv_call(ops, p, slice(0, 2), True, cs16)
    p.check_qkv(qq, kk, vv, checks, pp, slice(0, 2), True, cs16[:2], "the correct call after the refusals")

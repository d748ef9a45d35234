"""The bounds and frames of tests/test_gpu_batch_gemm_elements.py, proved on the CPU before they judge bgemm_dma_kernel.

A model of the kernel's arithmetic (decode_batch.hip): per wave the fp32 sum of its k-blocks (wave w: w, w + 8, ...), the eight partials added in
wave order, then bgemm_epilogue's sequence of bf16 roundings for each of the three modes, stored through raw offsets into the framed buffers as the
kernel forms them.
  - Neither too tight: the model stays inside the bound at every (n, N, K) and every head shape the GPU file runs (worst err / bound <= 1).
  - Nor too loose: each fault below falls outside the bound, or breaks a frame, and the worst offenders named lie where it acts:
      the last k-block of one wave's share dropped (K = 576, wave 0: k-block 8)      bound, in that item's 16 columns
      the item two grid steps earlier written instead (a stale parity buffer)          bound, in the third item of block 0 (N = 8200: item 512)
      rows m and m + 4 swapped (a lane group)                                          bound in those rows at n = 16; at n = 9 row 12 is a row
                                                                                       beyond the batch, and the frame of the 16-row output names it
      the clamped last tile's columns all taken from weight row N - 1                  bound, in columns 16 .. 18 of N = 20 (19 is right)
      RoPE with sin and cos swapped for one head                                       bound, in that head's columns
      K written at pos + 1                                                             the cache frame (a row that is not the row's own) and the
                                                                                       unwritten row pos (still the pattern: non-finite)
      a row >= n stored                                                                the output frame; the cache frame for its K/V
      a row with pos >= max_ctx stored                                                 the cache frame (the next kv head, the next slot or the guard)
  - The silu_f model in fp32 against fp64 stays inside silu_f_rel_err."""
import ast
import functools

import pytest
import torch

from tests.gpu_util import (BF16_U, assert_elementwise, assert_qkv_outputs, bgemm_acc_bound, bgemm_gateup_bound, bgemm_plain_bound, bgemm_qkv_bound,
                            framed_cache, framed_out_rows, rope_table, silu_f_rel_err)
from tests.test_gpu_batch_gemm_elements import HEADS, MAX_CTX, PLAIN_SHAPES, POS16, QKV_CASES, ROPE_POS16

G = 4


def _bf(t):
    return t.to(torch.bfloat16).float()


def _silu_f(x):
    return x / (1.0 + torch.exp(-x))                       # fp32 in, fp32 out: common.h silu_f


def _sums(x, w, drop=None, stale=None, clamp_to_last=False):
    """[rows, N] fp32 as the kernel sums: 8 wave partials over k-blocks wave, wave + 8, ..., added in wave order.  Faults: drop = (wave, item): that
    wave loses its last k-block in the item's 16 columns; stale = (item, from_item): the item's columns hold from_item's sums; clamp_to_last: every
    column of the clamped last tile is computed from weight row N - 1."""
    N, K = w.shape
    nkb = K // 64
    total = torch.zeros((x.shape[0], N))
    for wave in range(8):
        kbs = list(range(wave, nkb, 8))
        part = torch.zeros_like(total)
        for kb in kbs:
            p = x[:, kb * 64:(kb + 1) * 64].float() @ w[:, kb * 64:(kb + 1) * 64].float().t()
            if drop is not None and wave == drop[0] and kb == kbs[-1]:
                p[:, drop[1] * 16:drop[1] * 16 + 16] = 0
            part += p
        total += part
    if stale is not None:
        item, src = stale
        width = min(16, N - item * 16)
        total[:, item * 16:item * 16 + width] = total[:, src * 16:src * 16 + width]
    if clamp_to_last and N % 16:
        total[:, N // 16 * 16:] = total[:, N - 1:N]
    return total


@functools.lru_cache(maxsize=2)
def _problem(N, K, w2=False):
    """16 rows of everything, on the CPU, drawn as the GPU file draws them -> dict."""
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn(16, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    p = dict(x=x, w=w, bias=torch.randn(N, generator=g).to(torch.bfloat16), res=torch.randn(16, N, generator=g).to(torch.bfloat16))
    xd = x.double()
    p["core"], p["core_abs"], p["sums"] = xd @ w.double().t(), xd.abs() @ w.double().abs().t(), _sums(x, w)
    if w2:
        u = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
        p["w2"], p["core2"], p["core2_abs"], p["sums2"] = u, xd @ u.double().t(), xd.abs() @ u.double().abs().t(), _sums(x, u)
    return p


def _plain_model(sums, bias, res, out_f32=False):
    """decode_batch.hip:100-104"""
    v = sums if bias is None else sums + bias.float()
    if out_f32:
        return v
    if res is not None:
        v = _bf(v) + res.float()
    return v.to(torch.bfloat16)


def _gateup_model(sums, sums2):
    """decode_batch.hip:57-58"""
    return (_bf(_silu_f(_bf(sums))) * _bf(sums2)).to(torch.bfloat16)


def _qkv_model(sums, bias, cs, nq, nkv, hd, swap_head=None):
    """decode_batch.hip:72-77 -> [rows, N] bf16 in q | k | v order.  swap_head: that head reads its sin where its cos lies and the reverse."""
    n, half = sums.shape[0], hd // 2
    v = _bf(sums if bias is None else sums + bias.float())
    out = v.clone()
    rope = (nq + nkv) * hd
    v4 = v[:, :rope].reshape(n, -1, 2, half)
    lo, hi = v4[:, :, 0], v4[:, :, 1]
    c, s = cs[:, None, :half].expand(n, nq + nkv, half).clone(), cs[:, None, half:].expand(n, nq + nkv, half).clone()
    if swap_head is not None:
        c[:, swap_head], s[:, swap_head] = s[:, swap_head].clone(), c[:, swap_head].clone()
    oa = _bf(_bf(lo * c) + _bf(-hi * s))
    ob = _bf(_bf(hi * c) + _bf(lo * s))
    out[:, :rope] = torch.stack((oa, ob), 2).reshape(n, rope)
    return out.to(torch.bfloat16)


def _storage(view):
    return view.as_strided((view.untyped_storage().nbytes() // view.element_size(),), (1,), 0)


def _store_rows(view, vals, rows):
    """Row m of vals to row m of the 16-row view by its raw offset, as the kernel's store forms it (m * ld + column)."""
    flat = _storage(view)
    for m in rows:
        at = view.storage_offset() + m * view.stride(0)
        flat[at:at + vals.shape[1]] = vals[m]


def _offenders(exc):
    return ast.literal_eval(str(exc.value).split("of the worst: ")[1])


# ---- the model is inside every bound at every shape of the GPU file ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,K", PLAIN_SHAPES, ids=str)
def test_plain_model_is_inside_the_bound(n, N, K):
    p = _problem(N, K)
    r = slice(0, n)
    for bias, res in ((None, None), (p["bias"], None), (None, p["res"][r]), (p["bias"], p["res"][r])):
        b64, r64 = None if bias is None else bias.double(), None if res is None else res.double()
        ref, bound = bgemm_plain_bound(p["core"][r], p["core_abs"][r], K, b64, r64)
        assert assert_elementwise(_plain_model(p["sums"][r], bias, res), ref, bound, f"plain ({n}, {N}, {K})") <= 1.0
        ref, bound = bgemm_plain_bound(p["core"][r], p["core_abs"][r], K, b64, out_f32=True)
        assert assert_elementwise(_plain_model(p["sums"][r], bias, None, out_f32=True), ref, bound, f"plain fp32 ({n}, {N}, {K})") <= 1.0


def test_a_bf16_output_does_not_pass_as_an_fp32_one_nor_one_rounding_as_two():
    p = _problem(20, 576)
    ref, bound = bgemm_plain_bound(p["core"], p["core_abs"], 576, p["bias"].double(), out_f32=True)
    with pytest.raises(AssertionError, match="over the bound"):
        assert_elementwise(_plain_model(p["sums"], p["bias"], None).float(), ref, bound, "bf16 as fp32")
    # a residual that cancels the projection: the first rounding is 2^-8 |core + bias|, far above 2 * 2^-8 |ref|, and the bound admits it
    res = (-(p["sums"] + p["bias"].float()) * 0.99).to(torch.bfloat16)
    ref, bound = bgemm_plain_bound(p["core"], p["core_abs"], 576, p["bias"].double(), res.double())
    out = _plain_model(p["sums"], p["bias"], res)
    assert assert_elementwise(out, ref, bound, "cancelling residual") <= 1.0
    assert bool(((out.double() - ref).abs() > 2 * BF16_U * ref.abs() + bgemm_acc_bound(p["core_abs"] + p["bias"].double().abs() + res.double().abs(), 576)).any())


@pytest.mark.parametrize("n,N,K", PLAIN_SHAPES, ids=str)
def test_gateup_model_is_inside_the_bound(n, N, K):
    p = _problem(N, K, True)
    r = slice(0, n)
    ref, bound = bgemm_gateup_bound(p["core"][r], p["core_abs"][r], p["core2"][r], p["core2_abs"][r], K)
    assert assert_elementwise(_gateup_model(p["sums"][r], p["sums2"][r]), ref, bound, f"gate/up ({n}, {N}, {K})") <= 1.0


def test_silu_f_in_fp32_is_inside_its_error_term():
    x = torch.linspace(-30, 30, 200001, dtype=torch.float64).to(torch.bfloat16).float().unique()
    exact = x.double() / (1.0 + torch.exp(-x.double()))
    err = (_silu_f(x).double() - exact).abs()
    assert bool((err <= silu_f_rel_err(x.double().abs()) * exact.abs()).all())


def _qkv_problem(heads, K, use_bias):
    nq, nkv, hd = heads
    p = _problem((nq + 2 * nkv) * hd, K)
    cs = rope_table(ROPE_POS16, hd)
    bias = p["bias"] if use_bias else None
    return p, cs, bias


@pytest.mark.parametrize("heads,n,K,use_bias", QKV_CASES, ids=str)
def test_qkv_model_is_inside_the_bound_and_the_frames(heads, n, K, use_bias):
    nq, nkv, hd = heads
    p, cs, bias = _qkv_problem(heads, K, use_bias)
    ref, bound = bgemm_qkv_bound(p["core"][:n], p["core_abs"][:n], K, None if bias is None else bias.double(), cs[:n].double(), nq, nkv, hd)
    out = _qkv_model(p["sums"][:n], bias, cs[:n], nq, nkv, hd)
    q, kc, vc, checks = _qkv_buffers(heads, n)
    _qkv_store(out, q, kc, vc, POS16, n, heads)
    assert assert_qkv_outputs(q, kc, vc, checks, POS16[:n], n, ref, bound, nq, nkv, hd, f"qkv model {heads} n={n} K={K}") <= 1.0


# ---- q|k|v stores by raw offset ---------------------------------------------------------------------------------------------------------------------------------
def _qkv_buffers(heads, n):
    nq, nkv, hd = heads
    q, check_q = framed_out_rows(n, nq * hd, 8, G, device="cpu")
    kc, check_k = framed_cache(nkv, MAX_CTX, hd, device="cpu")
    vc, check_v = framed_cache(nkv, MAX_CTX, hd, device="cpu")
    return q, kc, vc, (check_q, check_k, check_v)


def _qkv_store(out, q, kc, vc, pos, rows, heads, k_shift=0, ctx_guard=True):
    """bgemm_epilogue's mode 2 stores (decode_batch.hip:79-89) for rows 0 .. rows - 1 of out: q by m * ldq, K/V by m * slot_stride +
    (kv head * max_ctx + pos) * head_dim.  Faults: k_shift moves K's row; ctx_guard = False drops the `pos < max_ctx` test."""
    nq, nkv, hd = heads
    QS, KS = nq * hd, nkv * hd
    _store_rows(q, out[:, :QS], range(rows))
    for cache, c0, shift in ((kc, QS, k_shift), (vc, QS + KS, 0)):
        flat = _storage(cache)
        for m in range(rows):
            if ctx_guard and pos[m] >= MAX_CTX:
                continue
            for h in range(nkv):
                at = cache.storage_offset() + m * cache.stride(0) + (h * MAX_CTX + pos[m] + shift) * hd
                if at + hd <= flat.numel():                                                  # (beyond the allocation: someone else's memory)
                    flat[at:at + hd] = out[m, c0 + h * hd:c0 + (h + 1) * hd]


# ---- every injected fault is rejected where it acts -----------------------------------------------------------------------------------------------------------
def _expect_over_bound(out, ref, bound, rows, cols, what):
    with pytest.raises(AssertionError, match="over the bound") as ei:
        assert_elementwise(out, ref, bound, what)
    worst = _offenders(ei)
    assert all(r in rows and c in cols for r, c, _ in worst), (what, worst)


def test_lost_last_k_block_of_one_wave_is_over_the_bound_in_its_item():
    n, N, K, item = 16, 4100, 576, 3
    p = _problem(N, K, True)
    bad = _sums(p["x"], p["w"], drop=(0, item))                                              # wave 0 owns k-blocks 0 and 8: 8 is lost
    cols = range(item * 16, item * 16 + 16)
    ref, bound = bgemm_plain_bound(p["core"], p["core_abs"], K, p["bias"].double(), p["res"].double())
    _expect_over_bound(_plain_model(bad, p["bias"], p["res"]), ref, bound, range(n), cols, "plain, lost k-block")
    ref, bound = bgemm_plain_bound(p["core"], p["core_abs"], K, None, out_f32=True)
    _expect_over_bound(_plain_model(bad, None, None, out_f32=True), ref, bound, range(n), cols, "fp32, lost k-block")
    ref, bound = bgemm_gateup_bound(p["core"], p["core_abs"], p["core2"], p["core2_abs"], K)
    _expect_over_bound(_gateup_model(bad, p["sums2"]), ref, bound, range(n), cols, "gate/up, lost k-block of the gate")
    _expect_over_bound(_gateup_model(p["sums"], _sums(p["x"], p["w2"], drop=(0, item))), ref, bound, range(n), cols, "gate/up, lost k-block of up")
    # the whole-row rel-L2 of the steps' tests does not see it: 16 columns of 4100 lost one k-block of nine
    out = _plain_model(bad, p["bias"], p["res"]).double()
    assert float((out - (p["core"] + p["bias"].double() + p["res"].double())).norm() / out.norm()) < 1.5e-2


def test_stale_parity_buffer_is_over_the_bound_in_the_third_item_of_block_0():
    n, N, K = 9, 8200, 64
    p = _problem(N, K)
    bad = _sums(p["x"], p["w"], stale=(512, 0))[:n]                                          # items 0, 256, 512 on block 0: 512 reads 0's buffer
    ref, bound = bgemm_plain_bound(p["core"][:n], p["core_abs"][:n], K, p["bias"].double())
    _expect_over_bound(_plain_model(bad, p["bias"], None), ref, bound, range(n), range(8192, 8200), "stale parity")
    assert assert_elementwise(_plain_model(p["sums"][:n], p["bias"], None), ref, bound, "clean") <= 1.0


def test_swapped_lane_groups_are_over_the_bound_or_break_the_frame():
    N, K = 20, 448
    p = _problem(N, K)
    out = _plain_model(p["sums"], p["bias"], p["res"])
    ref, bound = bgemm_plain_bound(p["core"], p["core_abs"], K, p["bias"].double(), p["res"].double())
    bad = out.clone(); bad[8:12], bad[12:16] = out[12:16], out[8:12]
    _expect_over_bound(bad, ref, bound, range(8, 16), range(N), "rows 8-11 and 12-15 swapped, n = 16")
    # n = 9: row 8's values land in row 12, a row beyond the batch: the bound sees row 8 (never written: the pattern), the frame sees row 12
    n = 9
    view, check = framed_out_rows(n, N, 8, G, device="cpu")
    _store_rows(view, out, range(8))
    _store_rows(view, torch.cat((out[:12], out[8:9])), [12])
    with pytest.raises(AssertionError, match=r"non-finite.*\(8, 0\)"):
        assert_elementwise(view[:n], ref[:n], bound[:n], "row 8 unwritten")
    with pytest.raises(AssertionError, match=r"outside the \[9, 20\] view.*\(12, 0\)"):
        check()


def test_clamped_last_tile_read_from_row_n_minus_1_is_over_the_bound():
    n, N, K = 5, 20, 512
    p = _problem(N, K, True)
    bad = _sums(p["x"], p["w"], clamp_to_last=True)[:n]
    ref, bound = bgemm_plain_bound(p["core"][:n], p["core_abs"][:n], K)
    _expect_over_bound(_plain_model(bad, None, None), ref, bound, range(n), range(16, 19), "clamped tile, plain")
    ref, bound = bgemm_gateup_bound(p["core"][:n], p["core_abs"][:n], p["core2"][:n], p["core2_abs"][:n], K)
    _expect_over_bound(_gateup_model(p["sums"][:n], _sums(p["x"], p["w2"], clamp_to_last=True)[:n]), ref, bound, range(n), range(16, 19), "clamped tile, up")


def test_a_stored_row_beyond_the_batch_breaks_the_output_frame():
    n, N, K = 5, 20, 512
    p = _problem(N, K)
    out = _plain_model(p["sums"], p["bias"], None)
    for dtype in (torch.bfloat16, torch.float32):
        view, check = framed_out_rows(n, N, 8, G, dtype=dtype, device="cpu")
        _store_rows(view, out.to(dtype), range(n))
        check()
        _store_rows(view, out.to(dtype), [n])
        with pytest.raises(AssertionError, match=r"outside the \[5, 20\] view.*\(5, 0\)"):
            check()
    # n = 16: the row behind the view is a guard row
    view, check = framed_out_rows(16, N, 8, G, device="cpu")
    _store_rows(view, torch.cat((out, out[:1])), range(17))
    with pytest.raises(AssertionError, match=r"\(16, 0\)"):
        check()
    # a column beyond N in the ld padding
    view, check = framed_out_rows(n, N, 8, G, device="cpu")
    _store_rows(view, torch.cat((out, out[:, :1]), 1), range(n))
    with pytest.raises(AssertionError, match=r"\(0, 20\)"):
        check()


@pytest.mark.parametrize("heads", HEADS, ids=str)
def test_qkv_faults_are_rejected(heads):
    nq, nkv, hd = heads
    n, K = 9, 576
    QS, KS = nq * hd, nkv * hd
    p, cs, bias = _qkv_problem(heads, K, True)
    ref, bound = bgemm_qkv_bound(p["core"][:n], p["core_abs"][:n], K, bias.double(), cs[:n].double(), nq, nkv, hd)
    good = _qkv_model(p["sums"], bias, cs, nq, nkv, hd)
    pos = POS16[:n]
    what = f"qkv {heads}"

    def run(out=good, rows=n, **faults):
        q, kc, vc, checks = _qkv_buffers(heads, n)
        _qkv_store(out, q, kc, vc, POS16, rows, heads, **faults)
        return assert_qkv_outputs(q, kc, vc, checks, pos, n, ref, bound, nq, nkv, hd, what)

    assert run() <= 1.0
    # sin and cos swapped for one q head and for the k head: over the bound inside that head (q) / its cache rows (K)
    head = nq - 1
    with pytest.raises(AssertionError, match=f"{what} q.*over the bound".replace("(", r"\(").replace(")", r"\)")) as ei:
        run(_qkv_model(p["sums"], bias, cs, nq, nkv, hd, swap_head=head))
    assert all(head * hd <= c < (head + 1) * hd for _, c, _ in _offenders(ei))
    with pytest.raises(AssertionError, match="K rows.*over the bound") as ei:
        run(_qkv_model(p["sums"], bias, cs, nq, nkv, hd, swap_head=nq))
    assert all(c < hd for _, c, _ in _offenders(ei))
    # the bias of one V column lost: over the bound in that column of the V rows
    nobias = _qkv_model(p["sums"], torch.cat((bias[:QS + KS + 3], bias[:1] * 0, bias[QS + KS + 4:])), cs, nq, nkv, hd)
    with pytest.raises(AssertionError, match="V rows.*over the bound") as ei:
        run(nobias)
    assert all(c == 3 for _, c, _ in _offenders(ei))
    # K at pos + 1: the row's own cache row keeps the pattern (non-finite); with the values checked out of the way, the frame names the other row
    with pytest.raises(AssertionError, match="K rows.*non-finite"):
        run(k_shift=1)
    q, kc, vc, checks = _qkv_buffers(heads, n)
    _qkv_store(good, q, kc, vc, POS16, n, heads, k_shift=1)
    checks[2](pos, n)
    with pytest.raises(AssertionError, match=r"KV cache.*first at \(slot, kv head, position, column\) \[\(0, 0, 4, 0\)"):
        checks[1](pos, n)
    # a row >= n stored: q's frame and the cache's (slot 9, position 6)
    q, kc, vc, checks = _qkv_buffers(heads, n)
    _qkv_store(good, q, kc, vc, POS16, n + 1, heads)
    with pytest.raises(AssertionError, match=r"outside the \[9, \d+\] view.*\(9, 0\)"):
        checks[0]()
    with pytest.raises(AssertionError, match=r"KV cache.*\[\(9, 0, 6, 0\)"):
        checks[1](pos, n)
    # rows with pos >= max_ctx stored: row 1 (pos 8) lands in the next kv head's row 0 or, from the last head, in the next slot; row 3 (pos 13) alike
    q, kc, vc, checks = _qkv_buffers(heads, n)
    _qkv_store(good, q, kc, vc, POS16, n, heads, ctx_guard=False)
    checks[0]()
    for c in checks[1:]:
        with pytest.raises(AssertionError, match="KV cache"):
            c(pos, n)
    # ... the last slot's overflow reaches the guard slot behind the cache (n = 16, row 13 at pos 13)
    q, kc, vc, checks = _qkv_buffers(heads, 16)
    _qkv_store(good, q, kc, vc, POS16, 16, heads, ctx_guard=False)
    with pytest.raises(AssertionError, match="KV cache"):
        checks[1](POS16, 16)


def test_the_operator_entries_are_bound_and_declared():
    import os
    import re
    from vila_amd import _lib, ops
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vila_hip.h")) as f:
        header = f.read()
    for name, n_args in (("vila_gemm_batch_bf16", 15), ("vila_qkv_batch_bf16", 18)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None and decl.group(1).count(",") == n_args - 1, f"{name}: declaration in include/vila_hip.h"
    assert callable(ops.gemm_batch) and callable(ops.qkv_batch)

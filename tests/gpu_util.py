import json
import os

import torch

# "grads cosine >= 0.999" — the stated bound of every model-gradient comparison (bf16 HIP step vs fp32 autograd).
# A tensor that cannot meet it carries a per-tensor exception at its call site, with the measured value and the reason.
GRAD_COS_MIN = 0.999


def grad_cos(test: str, name: str, got: torch.Tensor, ref: torch.Tensor) -> float:
    """Cosine of a gradient tensor against its fp32 reference.  With VILA_DUMP_COS=<file> every measured value is appended as a JSON line
    (what the per-tensor exceptions in the tests were read from)."""
    cos = float(torch.nn.functional.cosine_similarity(got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten(), dim=0))
    path = os.environ.get("VILA_DUMP_COS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": test, "tensor": name, "cos": cos, "ref_norm": float(ref.norm()), "numel": ref.numel()}) + "\n")
    return cos


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def randn_bf16(*shape, seed=0, scale=1.0, device="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device=device, dtype=torch.bfloat16)


def margin_aware_ids(lg, lg_o, ids_o, free_ids=None):
    """SURVEY §8c id rule.  `lg` [n,V]: teacher-forced GPU logits (the oracle's ids were fed), `lg_o` / `ids_o`: the oracle's.  At every
    step whose oracle top-1/top-2 margin exceeds 4x the observed max-abs logit error the argmax must be bit-exact; `free_ids` (a
    free-running greedy run of the same model) must equal the oracle's ids up to the first non-decisive step — until then it was fed
    exactly the teacher-forced inputs.  Returns the decisive mask."""
    import torch
    lg, lg_o = lg.detach().float().cpu(), lg_o.detach().float().cpu()
    err = float((lg - lg_o).abs().max())
    top2 = lg_o.topk(2, -1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 4 * err
    assert bool(decisive.any()), f"no decisive step (err {err:.3e}, margins {(top2[:, 0] - top2[:, 1]).tolist()})"
    got = lg.argmax(-1)
    assert torch.equal(got[decisive], ids_o[decisive]), f"ids {got.tolist()} vs oracle {ids_o.tolist()} (err {err:.3e}, decisive {decisive.tolist()})"
    if free_ids is not None:
        free_ids = free_ids.detach().cpu().reshape(-1)
        nd = (~decisive).nonzero().flatten()
        k = int(nd[0]) if nd.numel() else len(ids_o)
        assert torch.equal(free_ids[:k], ids_o[:k]), f"free-running ids {free_ids.tolist()} vs oracle {ids_o.tolist()} (first {k} must match)"
    return decisive


def attn_ref(q, k, v, causal, cu=None, scale=None, return_lse=False):
    """fp32 attention reference: softmax(scale * Q K^T + mask) V per sequence (`cu` = cu_seqlens, None = one sequence), GQA: q head h reads
    kv head h // (Hq / Hkv); scale defaults to D^-0.5.  Computed per sequence and kv head so that the fp32 score matrices of long shapes stay
    a few GB.  -> o [T, Hq, D] fp32 (+ lse [Hq, T] fp32, the natural-log sum of exp(scale * s) over the visible keys)."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    out = torch.zeros((T, Hq, D), device=q.device, dtype=torch.float32)
    lse = torch.zeros((Hq, T), device=q.device, dtype=torch.float32)
    bounds = [0, T] if cu is None else cu.tolist()
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b == a:
            continue
        future = torch.triu(torch.ones(b - a, b - a, dtype=torch.bool, device=q.device), 1) if causal else None
        for g in range(Hkv):
            hs = slice(g * G, (g + 1) * G)
            s = torch.einsum("qhd,kd->hqk", q[a:b, hs].float(), k[a:b, g].float()) * scale
            if causal:
                s = s.masked_fill(future, float("-inf"))
            lse[hs, a:b] = torch.logsumexp(s, -1)
            out[a:b, hs] = torch.einsum("hqk,kd->qhd", torch.softmax(s, -1), v[a:b, g].float())
    return (out, lse) if return_lse else out


def attn_ref_grads(q, k, v, do, causal, cu=None, scale=None):
    """fp32 autograd through attn_ref's formula, one kv head (and its q-head group) at a time.  -> o, dq, dk, dv (fp32)."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    bounds = [0, T] if cu is None else cu.tolist()
    o = torch.zeros((T, Hq, D), device=q.device, dtype=torch.float32)
    dq, dk, dv = torch.zeros_like(o), torch.zeros((T, Hkv, D), device=q.device, dtype=torch.float32), torch.zeros((T, Hkv, D), device=q.device, dtype=torch.float32)
    for g in range(Hkv):
        hs = slice(g * G, (g + 1) * G)
        qf = q[:, hs].float().detach().requires_grad_(True)
        kf = k[:, g].float().detach().requires_grad_(True)
        vf = v[:, g].float().detach().requires_grad_(True)
        outs = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            s = torch.einsum("qhd,kd->hqk", qf[a:b], kf[a:b]) * scale
            if causal:
                s = s.masked_fill(torch.triu(torch.ones(b - a, b - a, dtype=torch.bool, device=q.device), 1), float("-inf"))
            outs.append(torch.einsum("hqk,kd->qhd", torch.softmax(s, -1), vf[a:b]))
        og = torch.cat(outs, 0)
        og.backward(do[:, hs].float())
        o[:, hs], dq[:, hs], dk[:, g], dv[:, g] = og.detach(), qf.grad, kf.grad, vf.grad
    return o, dq, dk, dv


# ---- planted-key inputs for the decode attentions (tests/test_decode_probe_cpu.py, tests/test_gpu_decode_keys.py) -------------------------
# With i.i.d. random Q/K/V one key of L carries about 1/L of a head's softmax weight, so a key lost or admitted at a chunk, slice or capacity
# boundary moves the output by less than the tests' bound once L is a few hundred.  A PLANTED key is alpha * q of one target query head per kv
# head: its score alpha |q|^2 / sqrt(128) is about 22 at alpha = 2 against N(0, 1) for the random keys, so it takes essentially all of that
# head's weight and the head returns that key's (random) V row.  Lose the key or admit one too many and the target heads move by O(|V|).
def probe_targets(kv: int, G: int):
    """The target query head of every kv head: another member of the group for each (kv head h -> head h * G + h % G)."""
    return [h * G + h % G for h in range(kv)]


def plant_keys(k_slot: torch.Tensor, q_row: torch.Tensor, keys, alpha=2.0) -> None:
    """In place: k_slot [kv, C, 128] bf16 gets, for every kv head h, rows `keys` = bf16(alpha * q_row[target head of h]) (q_row [nq, 128] bf16);
    alpha a number or one per key.  The V rows stay as they are."""
    kv, G = k_slot.shape[0], q_row.shape[0] // k_slot.shape[0]
    keys = list(keys)
    alphas = [float(alpha)] * len(keys) if not hasattr(alpha, "__len__") else [float(a) for a in alpha]
    for h, t in enumerate(probe_targets(kv, G)):
        for key, a in zip(keys, alphas):
            k_slot[h, key] = (a * q_row[t].float()).to(torch.bfloat16)


def staircase_alphas(q_row: torch.Tensor, kv: int, n_keys: int, step: float = 9.0, alpha0: float = 2.0):
    """alpha of planted key j = alpha0 + j * c with c chosen so that the score alpha |q|^2 / sqrt(128) of EVERY kv head's target rises by at least
    `step` per key (c from the smallest |q_t|^2): key j then outweighs all earlier ones by e^step."""
    G = q_row.shape[0] // kv
    n2 = min(float(q_row[t].float().pow(2).sum()) for t in probe_targets(kv, G))
    c = step * 128 ** 0.5 / n2
    return [alpha0 + j * c for j in range(n_keys)]


def decode_attn_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, visible: torch.Tensor, scale=None) -> torch.Tensor:
    """fp32 softmax over exactly the visible keys: q [n, nq, 128], k / v [n or 1, kv, C, 128] (row i reads slot i, or all rows the one slot),
    visible [n, C] bool -> o [n, nq, 128] fp32.  One kv head at a time, nothing expanded."""
    n, nq, D = q.shape
    kv = k.shape[1]
    G = nq // kv
    scale = D ** -0.5 if scale is None else scale
    out = torch.empty((n, nq, D), dtype=torch.float32, device=q.device)
    hide = ~visible[:, None, :]
    assert k.shape[0] in (1, n) and k.shape == v.shape and visible.shape == (n, k.shape[2])
    for h in range(kv):
        kh, vh = k[:, h].float().expand(n, -1, -1), v[:, h].float().expand(n, -1, -1)      # (a view: one slot serves every row)
        s = torch.einsum("ngd,ncd->ngc", q[:, h * G:(h + 1) * G].float(), kh) * scale
        p = torch.softmax(s.masked_fill(hide, float("-inf")), -1)
        out[:, h * G:(h + 1) * G] = torch.einsum("ngc,ncd->ngd", p, vh)
    return out


def visible_upto(lens, C: int, device="cpu") -> torch.Tensor:
    """[n, C] bool: row i sees keys 0 .. lens[i] - 1."""
    return torch.arange(C, device=device)[None, :] < torch.as_tensor(list(lens), device=device)[:, None]


# ---- element-wise GEMM checks and framed buffers (tests/test_gemm_bound_cpu.py proves them, tests/test_gpu_gemm_elements.py uses them) ----------
# A whole-matrix rel-L2 below 4e-3 leaves a factor 2.4 over the floor of a correct kernel (one bf16 rounding, 1.66e-3), spread over every
# element: a fault confined to one row, column or tile corner fits inside it.  The bound below is per element and derived, not measured.
BF16_U = 2.0 ** -8          # unit roundoff of bf16 under round-to-nearest
FP32_U = 2.0 ** -24         # unit roundoff of fp32
FRAME_PATTERN = {2: 0x7FA5, 4: 0x7FC0A5A5, 1: 0x5A}       # per element size: a NaN with a payload (bf16, fp32) / a byte


def gemm_elem_bound(ref64: torch.Tensor, absprod64: torch.Tensor, K: int, roundings: int = 1, extra_fp32_ops: int = 2) -> torch.Tensor:
    """Per-element bound on |out - ref| for out = bf16-rounded fp32 sum of K products (+ bias + residual):
        roundings * 2^-8 * |ref|  +  (1 + 2^-8) * (K + extra_fp32_ops) * 2^-24 * absprod
    `ref64`: the fp64 result on the same inputs; `absprod64`: |A| @ |W|^T + |bias| + |residual| in fp64, the magnitudes the kernel sums.  The
    second term is the textbook bound on an fp32 sum of K products in ANY order (split-K, sliced rings and the hybrid tail only reorder), the
    factor (1 + 2^-8) carries it through the final rounding.  roundings = 0: fp32 output; 2: the projection is rounded before the residual add."""
    return roundings * BF16_U * ref64.abs() + (1.0 + BF16_U) * (K + extra_fp32_ops) * FP32_U * absprod64


def assert_elementwise(out: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """Every element finite and |out - ref64| <= bound.  A failure states the count, the worst err / bound and the (row, col) of the worst few
    offenders, so that it names the tile.  -> the worst err / bound."""
    o = out.detach().double()
    assert o.shape == ref64.shape == bound.shape, (tuple(o.shape), tuple(ref64.shape), tuple(bound.shape))
    bad = ~torch.isfinite(o)
    n_bad = int(bad.sum())
    if n_bad:
        at = [tuple(int(i) for i in rc) for rc in bad.nonzero()[:8].tolist()]
        raise AssertionError(f"{what}: {n_bad} non-finite elements of {o.numel()}, first at (row, col) {at}")
    err = (o - ref64).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    over = ratio > 1.0
    n_over = int(over.sum())
    if n_over:
        top = ratio.flatten().topk(min(8, n_over))
        ncol = o.shape[-1]
        at = [(int(i) // ncol, int(i) % ncol, round(float(v), 2)) for v, i in zip(top.values.tolist(), top.indices.tolist())]
        raise AssertionError(f"{what}: {n_over} of {o.numel()} elements over the bound, worst err / bound {worst:.3g}; (row, col, ratio) of the worst: {at}")
    return worst


def _int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _pattern_of(t: torch.Tensor) -> int:
    p = FRAME_PATTERN[t.element_size()]
    return p - (1 << 32) if p >= (1 << 31) else p


def _frame_check(buf: torch.Tensor, r0: int, rows: int, cols: int, what: str):
    def check():
        iv = _int_view(buf).clone()
        iv[r0:r0 + rows, :cols] = _pattern_of(buf)
        hit = iv != _pattern_of(buf)
        n = int(hit.sum())
        if n:
            at = [(int(r) - r0, int(c)) for r, c in hit.nonzero()[:8].tolist()]
            raise AssertionError(f"{what}: {n} elements outside the [{rows}, {cols}] view were written; first at (row, col) relative to the view {at}")
    return check


def framed_out(M: int, N: int, ld_pad: int, guard_rows: int, dtype=torch.bfloat16, device="cuda", fill: torch.Tensor = None):
    """-> (view, check): the view is rows [g, g + M), columns [0, N) of a [(M + 2 g), N + ld_pad] buffer pre-filled with a fixed non-zero bit
    pattern (a NaN with a payload); check() asserts that every element outside the view still holds it bit for bit.  `fill` [M, N]: the view's
    initial values (the residual stream of an in-place GEMM).  The caller keeps ld = N + ld_pad and g * ld 16-byte aligned."""
    g, ld = guard_rows, N + ld_pad
    buf = torch.empty((M + 2 * g, ld), dtype=dtype, device=device)
    _int_view(buf).fill_(_pattern_of(buf))
    view = buf[g:g + M, :N]
    if fill is not None:
        view.copy_(fill)
    assert (ld * buf.element_size()) % 8 == 0 and view.data_ptr() % 16 == 0, (M, N, ld_pad, guard_rows)
    return view, _frame_check(buf, g, M, N, f"output frame [{M}, {N}] ld {ld}")


def framed_operand(t: torch.Tensor, ld_pad: int = 0, guard_rows: int = 0, pad=float("nan")) -> torch.Tensor:
    """The same values as a view of a larger buffer whose padding columns and guard rows hold `pad` (NaN; 127 for int8): a read outside the operand
    that reaches the result shows there.  1-D (bias, scales): `pad` on both sides, the view at an offset that is a multiple of 8 elements."""
    if t.dim() == 1:
        off = 8 * max(1, guard_rows)
        buf = torch.full((t.numel() + 2 * off,), pad, dtype=t.dtype, device=t.device)
        view = buf[off:off + t.numel()]
    else:
        R, C = t.shape
        buf = torch.full((R + 2 * guard_rows, C + ld_pad), pad, dtype=t.dtype, device=t.device)
        view = buf[guard_rows:guard_rows + R, :C]
    view.copy_(t)
    return view


def framed_ws(n_bytes: int, device="cuda", guard_bytes: int = 4096):
    """-> (ws, check): a uint8 workspace of exactly n_bytes with a patterned guard in front of it and behind it; check() asserts both guards intact."""
    buf = torch.full((n_bytes + 2 * guard_bytes,), FRAME_PATTERN[1], dtype=torch.uint8, device=device)
    ws = buf[guard_bytes:guard_bytes + n_bytes]

    def check():
        for name, part, base in (("before", buf[:guard_bytes], -guard_bytes), ("past", buf[guard_bytes + n_bytes:], n_bytes)):
            hit = part != FRAME_PATTERN[1]
            if bool(hit.any()):
                raise AssertionError(f"workspace of {n_bytes} bytes: {int(hit.sum())} bytes written {name} it, first at byte offset {base + int(hit.nonzero()[0])}")
    return ws, check


# ---- the batched decode's skinny GEMM (vila_amd/csrc/decode_batch.hip bgemm_dma_kernel): per-element bounds of its three epilogues and frames with
# 16 rows of which n are used (tests/test_batch_gemm_bound_cpu.py proves them, tests/test_gpu_batch_gemm_elements.py uses them) -------------------
BGEMM_EXTRA_OPS = 10        # fp32 additions behind the K products: the 8 wave partials (decode_batch.hip:232-235), the bias and the residual


def bgemm_acc_bound(absprod64: torch.Tensor, K: int) -> torch.Tensor:
    """A(.): gemm_elem_bound's accumulation term alone, (1 + 2^-8) (K + 10) 2^-24 absprod, for an fp32 sum of K products in any order (eight waves'
    k-blocks round-robin, then the eight partials), bias and residual."""
    return gemm_elem_bound(absprod64, absprod64, K, roundings=0, extra_fp32_ops=BGEMM_EXTRA_OPS)


def bgemm_plain_bound(core64, core_abs64, K: int, bias64=None, res64=None, out_f32: bool = False):
    """Mode 0 (decode_batch.hip:100-104) -> (ref, bound).  fp32 output: v = sum + bias as summed, A only (the residual is not part of it).  bf16
    output without residual: one rounding, 2^-8 |ref| + A.  With residual: bfround(v) + residual, rounded again (line 103): 2^-8 |core + bias| for
    the first rounding at ITS magnitude, 2^-8 |ref| for the second, + A; not 2 * 2^-8 |ref|, which fails a correct kernel where the residual
    cancels the projection."""
    proj = core64 if bias64 is None else core64 + bias64
    absprod = core_abs64 if bias64 is None else core_abs64 + bias64.abs()
    if out_f32 or res64 is None:
        return proj, (0.0 if out_f32 else BF16_U) * proj.abs() + bgemm_acc_bound(absprod, K)
    ref = proj + res64
    return ref, BF16_U * proj.abs() + BF16_U * ref.abs() + bgemm_acc_bound(absprod + res64.abs(), K)


def silu_f_rel_err(x_abs: torch.Tensor) -> torch.Tensor:
    """Relative error of common.h silu_f(x) = x / (1.f + __expf(-x)) in fp32.  __expf(-x) is v_exp_f32(-x * log2 e): the product's rounding moves
    the exponent by at most |x| log2(e) 2^-24, that is the result by |x| 2^-24 of itself, and v_exp_f32 is good to 1 ulp = 2 * 2^-24; the sum
    1 + E passes E's error on times E / (1 + E) <= 1 and rounds once (2^-24); the division is good to 2.5 ulp = 5 * 2^-24 in its fast form
    (correctly rounded otherwise).  Together (|x| + 8) 2^-24."""
    return (x_abs + 8.0) * FP32_U


def bgemm_gateup_bound(g64, g_abs64, u64, u_abs64, K: int):
    """Mode 1 (decode_batch.hip:57-58): y = bf(bf(silu_f(bf(g))) * bf(u)), four roundings -> (ref, bound).  d_g = A_g + 2^-8 |g| bounds the rounded
    gate, d_u likewise; s = bf(silu_f(bf(g))) is off silu(g) by d_s = 1.1 d_g + 2^-8 |silu(g)| + silu_f's own error (1.1 >= max |silu'| = 1.0998;
    silu_f_rel_err at the rounded gate, of magnitude at most |silu(g)| + 1.1 d_g); the product of the two rounded factors is off by
    d_s (|u| + d_u) + |silu(g)| d_u, and the last rounding adds 2^-8 |ref|.  Terms of second order in 2^-8 beyond those written (2^-8 of a
    first-order term each, below 0.4 % of the bound) are left out, as the project's other bounds leave them out."""
    d_g = bgemm_acc_bound(g_abs64, K) + BF16_U * g64.abs()
    d_u = bgemm_acc_bound(u_abs64, K) + BF16_U * u64.abs()
    s = g64 / (1.0 + torch.exp(-g64))
    d_s = 1.1 * d_g + BF16_U * s.abs() + silu_f_rel_err(g64.abs() + d_g) * (s.abs() + 1.1 * d_g)
    ref = s * u64
    return ref, d_s * (u64.abs() + d_u) + s.abs() * d_u + BF16_U * ref.abs()


def bgemm_qkv_bound(core64, core_abs64, K: int, bias64, cs64, q_heads: int, kv_heads: int, head_dim: int):
    """Mode 2 (decode_batch.hip:72-77) -> (ref, bound), both [n, (q + 2 kv) * head_dim] in q | k | v column order.  cs64 [n, head_dim]: the table
    the kernel reads (cos | sin).  Every element is first lo = bf(sum + bias): d = A + 2^-8 |a + bias| (V heads stop here).  Q and K heads:
    lo' = bf(bf(lo c) + bf(-hi s)), hi' = bf(bf(hi c) + bf(lo s)).  First order F = |c| d_lo + |s| d_hi + 2^-8 (|a c| + |b s|) + 2^-8 |ref| (a, b:
    the biased sums of the element and of its partner; symmetric for hi').  Second order: the two product roundings and the last one act on values
    that already carry the earlier errors, each at most F, so 2 * 2^-8 F more; the fp32 add of the two rounded products rounds once, and the
    conversion reads that sum: below 4 * 2^-24 (|a c| + |b s|).  bound = (1 + 2^-7) F + 2^-22 (|a c| + |b s|)."""
    n = core64.shape[0]
    half = head_dim // 2
    proj = core64 if bias64 is None else core64 + bias64
    absprod = core_abs64 if bias64 is None else core_abs64 + bias64.abs()
    d = bgemm_acc_bound(absprod, K) + BF16_U * proj.abs()
    ref, bound = proj.clone(), d.clone()
    rope = (q_heads + kv_heads) * head_dim
    p4, d4 = proj[:, :rope].reshape(n, -1, 2, half), d[:, :rope].reshape(n, -1, 2, half)
    lo, hi, d_lo, d_hi = p4[:, :, 0], p4[:, :, 1], d4[:, :, 0], d4[:, :, 1]
    c, s = cs64[:, None, :half], cs64[:, None, half:]
    r_lo, r_hi = lo * c - hi * s, hi * c + lo * s
    m_lo, m_hi = (lo * c).abs() + (hi * s).abs(), (hi * c).abs() + (lo * s).abs()
    f_lo = c.abs() * d_lo + s.abs() * d_hi + BF16_U * m_lo + BF16_U * r_lo.abs()
    f_hi = c.abs() * d_hi + s.abs() * d_lo + BF16_U * m_hi + BF16_U * r_hi.abs()
    ref[:, :rope] = torch.stack((r_lo, r_hi), 2).reshape(n, rope)
    bound[:, :rope] = torch.stack(((1 + 2 * BF16_U) * f_lo + 4 * FP32_U * m_lo, (1 + 2 * BF16_U) * f_hi + 4 * FP32_U * m_hi), 2).reshape(n, rope)
    return ref, bound


def rope_table(positions, head_dim: int, theta: float = 1e6, device="cpu") -> torch.Tensor:
    """[n, head_dim] fp32, cos | sin of position * theta^(-2 d / head_dim), each rounded to bf16: the table bdec_prologue_kernel writes."""
    p = torch.as_tensor(list(positions), dtype=torch.float64, device=device)[:, None]
    inv = theta ** (-torch.arange(head_dim // 2, dtype=torch.float64, device=device) * 2.0 / head_dim)
    ang = p * inv[None, :]
    return torch.cat((torch.cos(ang), torch.sin(ang)), 1).to(torch.bfloat16).float().contiguous()


def framed_out_rows(n: int, N: int, ld_pad: int, guard_rows: int, rows: int = 16, dtype=torch.bfloat16, device="cuda", fill: torch.Tensor = None):
    """-> (view, check): framed_out for an output of `rows` rows of which only the first n may be written.  The view has all `rows` rows; check()
    asserts that everything outside its first n rows and N columns (rows n .. rows - 1, the ld padding, the guard rows) still holds the pattern.
    `fill` [n, N]: the initial values of the rows in use (an in-place residual)."""
    g, ld = guard_rows, N + ld_pad
    buf = torch.empty((rows + 2 * g, ld), dtype=dtype, device=device)
    _int_view(buf).fill_(_pattern_of(buf))
    view = buf[g:g + rows, :N]
    if fill is not None:
        view[:n].copy_(fill)
    return view, _frame_check(buf, g, n, N, f"output frame [{n} of {rows}, {N}] ld {ld}")


def framed_cache(kv_heads: int, max_ctx: int, head_dim: int, slots: int = 16, guard_slots: int = 1, device="cuda"):
    """-> (cache, check): a bf16 KV cache [slots][kv][max_ctx][head_dim] holding the frame pattern, between guard slots.  check(pos, n) asserts
    that the only elements that differ from the pattern lie in (slot m, every kv head, row pos[m]) of the rows m < n with pos[m] < max_ctx."""
    buf = torch.empty((slots + 2 * guard_slots, kv_heads, max_ctx, head_dim), dtype=torch.bfloat16, device=device)
    _int_view(buf).fill_(_pattern_of(buf))
    cache = buf[guard_slots:guard_slots + slots]

    def check(pos, n):
        allowed = torch.zeros(buf.shape[:3], dtype=torch.bool, device=buf.device)
        for m, p in enumerate(list(pos)[:n]):
            if 0 <= int(p) < max_ctx:
                allowed[guard_slots + m, :, int(p)] = True
        hit = (_int_view(buf) != _pattern_of(buf)) & ~allowed[..., None]
        k = int(hit.sum())
        if k:
            at = [(s - guard_slots, h, r, c) for s, h, r, c in hit.nonzero()[:8].tolist()]
            raise AssertionError(f"KV cache: {k} elements outside the rows' own (slot, position) were written; first at (slot, kv head, position, column) {at}")
    return cache, check


def cache_rows(cache: torch.Tensor, pos, n: int):
    """-> (rows [k, kv * head_dim], index): the cache rows (slot m, every kv head, pos[m]) of the k rows m < n with pos[m] < max_ctx, heads side
    by side as the q|k|v reference has them, and the list of those m."""
    idx = [m for m in range(n) if 0 <= int(pos[m]) < cache.shape[2]]
    if not idx:
        return cache.new_zeros((0, cache.shape[1] * cache.shape[3])), idx
    return torch.stack([cache[m, :, int(pos[m])].reshape(-1) for m in idx]), idx


def assert_qkv_outputs(q, kcache, vcache, frame_checks, pos, n: int, ref64, bound, q_heads: int, kv_heads: int, head_dim: int, what: str = "") -> float:
    """The checks of one q|k|v call: q [>= n, q * head_dim] and the rows' own cache rows element by element against ref / bound (an unwritten cache
    row still holds the pattern, a NaN, and fails as non-finite), then every frame (q's, and check(pos, n) of both caches).  -> worst err / bound."""
    QS, KS = q_heads * head_dim, kv_heads * head_dim
    worst = assert_elementwise(q[:n], ref64[:, :QS], bound[:, :QS], f"{what} q")
    for name, cache, c0 in (("K", kcache, QS), ("V", vcache, QS + KS)):
        rows, live = cache_rows(cache, pos, n)
        if live:
            worst = max(worst, assert_elementwise(rows, ref64[live, c0:c0 + KS], bound[live, c0:c0 + KS], f"{what} {name} rows of {live}"))
    check_q, check_k, check_v = frame_checks
    check_q(); check_k(pos, n); check_v(pos, n)
    return worst


# ---- the SFT operators of vila_amd/csrc/train.hip and the norms of elementwise.hip: per-element references and bounds -------------------------
# (tests/test_train_bound_cpu.py proves them, tests/test_gpu_train_elements.py uses them).  Every bound has the shape
#     roundings * 2^-8 * |ref|  +  (1 + 2^-8) * 2^-24 * sum_k c_k |term_k|  +  floor
# c_k: the number of fp32 roundings term k passes through (reduction depth + single operations), term_k: what the kernel adds for that element.
# The functions return (ref64, bound64, acc64): acc64 is the middle part alone, which the CPU file compares with the rounding part.
FTZ = 2.0 ** -126           # v_exp_f32 / v_rcp_f32 flush results below the smallest normal fp32; multiplied by what the result is scaled with


def f32(x: float) -> float:
    """The value a C float argument or literal takes."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def train_bound(ref64, acc64, roundings: int = 1, floor=FTZ):
    return roundings * BF16_U * ref64.abs() + (1.0 + BF16_U) * FP32_U * acc64 + floor


def bf16_round64(v64: torch.Tensor) -> torch.Tensor:
    return v64.to(torch.bfloat16).double()


def bf16_near_tie(v64: torch.Tensor, err64: torch.Tensor):
    """-> (near, ulp): whether v lies within err of a bf16 rounding tie (an odd multiple of half the spacing at |v|), and that spacing.  Only such
    an element may come out one inner ulp away when its fp32 value is rounded to bf16 before the next operation."""
    _, e = torch.frexp(v64.abs().clamp_min(FTZ))
    ulp = torch.ldexp(torch.ones_like(v64), e - 8)
    q = v64.abs() / ulp
    return ((q - q.floor()) - 0.5).abs() * ulp <= err64, ulp


def framed_flat(n: int, dtype=torch.bfloat16, device="cuda", guard: int = 64, fill: torch.Tensor = None):
    """-> (view, check): n contiguous elements between two guards of `guard` elements holding the frame pattern (the view too, unless `fill`);
    check() asserts both guards intact.  The view is 16-byte aligned when guard * element size is."""
    buf = torch.empty((n + 2 * guard,), dtype=dtype, device=device)
    _int_view(buf).fill_(_pattern_of(buf))
    view = buf[guard:guard + n]
    if fill is not None:
        view.copy_(fill.reshape(-1))

    def check():
        iv = _int_view(buf)
        for name, part, base in (("before", iv[:guard], -guard), ("past", iv[guard + n:], n)):
            hit = part != _pattern_of(buf)
            if bool(hit.any()):
                raise AssertionError(f"buffer of {n} elements: {int(hit.sum())} elements written {name} it, first at offset {base + int(hit.nonzero()[0])}")
    return view, check


# -- LayerNorm / RMSNorm forward (elementwise.hip) ---------------------------------------------------------------------------------------------
NORM_FWD_OPS = 8            # behind the reductions: / cols, + eps, rsqrtf (2 roundings), x - mean, * rstd, * w, + b  (elementwise.hip:39-41, 55, 72)


def norm_fwd_depth(cols: int) -> int:
    """Longest chain of fp32 additions of a row sum.  cols <= 1536: norm_wave_kernel<_, 3> (elementwise.hip:266, 278), a lane adds its
    ceil(nch / 64) chunks as 4 pairs each (lines 120-125: one add for the pair, one into s; chunks past the row add exact zeros), then 6 shuffle
    levels (lines 113-117).  Wider: norm_kernel / norm_block_lat_kernel, 256 lanes (lines 24-35, 200-206), 6 shuffle levels and the three adds
    of the four wave sums (common.h:40-45)."""
    nch = cols // 8
    lanes, levels = (64, 6) if cols <= 1536 else (256, 9)
    return 4 * _cdiv(nch, lanes) + 1 + levels


def norm_stats64(x64: torch.Tensor, rms: bool, eps: float):
    """-> mean [R, 1] (0 for RMSNorm), rstd [R, 1], xhat [R, C] in fp64; eps as the C float."""
    mean = torch.zeros_like(x64[:, :1]) if rms else x64.mean(-1, keepdim=True)
    rstd = ((x64 - mean).square().mean(-1, keepdim=True) + f32(eps)).rsqrt()
    return mean, rstd, (x64 - mean) * rstd


def layernorm_fwd_bound(x64, w64, b64, eps: float):
    """y = bf16((x - mean) rstd w + b), one rounding (elementwise.hip:72-75, 158-161, 239-242).  mag = |w| (rstd (|x| + mean|x|) + |xhat|) + |b|:
    the mean is off by depth 2^-24 mean|x| and x - mean rounds at |x| + |mean|, both scaled by rstd |w|; rstd is off by (depth / 2 + 4) 2^-24 of
    itself, which scales |w xhat|; b is added last.  Every term passes at most depth + NORM_FWD_OPS roundings.  The effect of the mean's error on
    the two-pass variance is (dmean / std)^2 < 2^-24 while mean|x| / std < 2^12 / depth (40 at the widest row; the inputs stay below 31)."""
    mean, rstd, xhat = norm_stats64(x64, False, eps)
    ref = xhat * w64 + (0.0 if b64 is None else b64)
    mag = w64.abs() * (rstd * (x64.abs() + x64.abs().mean(-1, keepdim=True)) + xhat.abs()) + (0.0 if b64 is None else b64.abs())
    acc = (norm_fwd_depth(x64.shape[-1]) + NORM_FWD_OPS) * mag
    return ref, train_bound(ref, acc), acc


def rmsnorm_fwd_bound(x64, w64, eps: float):
    """y = bf16(w * bf16(x rstd)), HF's two roundings (elementwise.hip:69-70, 155-156, 236-237) -> (ref, bound, acc, near).  The reference rounds
    in that order.  The product of two bf16 values is exact in fp32, so an element whose inner value x rstd is NOT within the fp32 error
    (depth + NORM_FWD_OPS) 2^-24 |x rstd| of a rounding tie must meet 2^-8 |ref| alone; a near-tie element may take one inner ulp, |w| ulp, more."""
    _, rstd, inner = norm_stats64(x64, True, eps)
    near, ulp = bf16_near_tie(inner, (norm_fwd_depth(x64.shape[-1]) + NORM_FWD_OPS) * FP32_U * inner.abs())
    ref = w64 * bf16_round64(inner)
    acc = torch.where(near, w64.abs() * ulp / FP32_U, torch.zeros_like(ref))
    return ref, train_bound(ref, acc), acc, near


# -- LayerNorm / RMSNorm backward (train.hip:301-524) ----------------------------------------------------------------------------------------------
NORM_BWD_OPS = 12           # single operations behind the reductions of dx: * inv_cols (x 2, inv_cols itself rounded), + eps, rsqrtf (2), x - mean,
                            # * rstd, xhat * mb, g - ma, - (xhat mb), * rstd and the product g xhat inside sb  (train.hip:423-458)


def norm_bwd_route(rows: int, cols: int, rms: bool, aligned: bool = True) -> dict:
    """The kernel launch_norm_bwd takes (train.hip:498-519) and its depths.  Wave kernel (RMS cols <= 4096, LayerNorm cols <= 1536, 16-byte
    aligned pointers, cols % 8 == 0): a lane adds 4 pairs per chunk over ceil(nch / 64) chunks (lines 419-423, 439-447), 6 shuffle levels; a
    wave adds its NB_ROWS = 3 rows into dwacc (lines 459-460), the four waves meet as (a + b) + (c + d) (line 480): blocks of 12 rows.  Generic
    kernel: a thread adds ceil(cols / 256) elements (lines 334, 348-352), 6 shuffle levels and 3 adds (block_sum4, lines 306-313); a block adds
    its 8 rows (line 364).  Then colpart_reduce_kernel (lines 240-253): ceil(parts / 4) partials in order, two tree levels, the old value."""
    wave = aligned and cols % 8 == 0 and ((rms and cols <= 4096) or (not rms and cols <= 1536))
    parts = _cdiv(rows, 12 if wave else 8)
    stat = 4 * _cdiv(cols // 8, 64) + 1 + 6 if wave else _cdiv(cols, 256) + 6 + 3
    return {"wave": wave, "parts": parts, "stat_depth": stat, "dw_depth": (3 + 2 if wave else 8) + _cdiv(parts, 4) + 2 + 1}


def norm_bwd_bounds(x64, w64, dy64, eps: float, rms: bool, route: dict, dw_old64=None, db_old64=None):
    """-> {"dx" / "dw" / "db": (ref, bound, acc)}.  dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w (exact in fp32).
    X = rstd (|x| + mean|x|) + |xhat| is what xhat's own error scales with (the forward's argument; RMSNorm: |xhat|, there is no mean).
    dx: mag = rstd (|g| + mean|g| + |xhat| mean|g xhat|) plus the carried error of xhat, rstd (|mb| X + |xhat| mean(|g| X)); a term passes at most
    1.5 reductions (rstd carries half the relative error of its sum, the square root's; mean(g) or mb a whole one) and NORM_BWD_OPS single operations.
    dw = sum_r dy xhat (+ old): dw_depth roundings on sum_r |dy xhat| (+ |old|), and xhat's error (stat_depth + NORM_FWD_OPS) on sum_r |dy| X.
    db = sum_r dy (+ old): dw_depth roundings on sum_r |dy| (+ |old|)."""
    mean, rstd, xhat = norm_stats64(x64, rms, eps)
    g = dy64 * w64
    ma = torch.zeros_like(mean) if rms else g.mean(-1, keepdim=True)
    mb = (g * xhat).mean(-1, keepdim=True)
    X = xhat.abs() if rms else rstd * (x64.abs() + x64.abs().mean(-1, keepdim=True)) + xhat.abs()
    dx = rstd * (g - ma - xhat * mb)
    mag = rstd * (g.abs() + (0.0 if rms else g.abs().mean(-1, keepdim=True)) + xhat.abs() * (g * xhat).abs().mean(-1, keepdim=True)
                  + mb.abs() * X + xhat.abs() * (g.abs() * X).mean(-1, keepdim=True))
    acc_dx = (1.5 * route["stat_depth"] + NORM_BWD_OPS) * mag
    out = {"dx": (dx, train_bound(dx, acc_dx), acc_dx)}
    dw = (dy64 * xhat).sum(0) + (0.0 if dw_old64 is None else dw_old64)
    acc_dw = route["dw_depth"] * ((dy64 * xhat).abs().sum(0) + (0.0 if dw_old64 is None else dw_old64.abs())) \
        + (route["stat_depth"] + NORM_FWD_OPS) * (dy64.abs() * X).sum(0)
    out["dw"] = (dw, train_bound(dw, acc_dw), acc_dw)
    if not rms:
        db = dy64.sum(0) + (0.0 if db_old64 is None else db_old64)
        acc_db = route["dw_depth"] * (dy64.abs().sum(0) + (0.0 if db_old64 is None else db_old64.abs()))
        out["db"] = (db, train_bound(db, acc_db), acc_db)
    return out


# -- cross entropy (train.hip:531-573) -----------------------------------------------------------------------------------------------------------
CE_IGNORE = -100


def ce_bounds(z64: torch.Tensor, labels: torch.Tensor, scale: float, loss0: float = 0.0):
    """z64 [n, V]: the fp32 logits as fp64 -> (dref, dbound, dacc, loss_ref, loss_bound).  dz = bf16((softmax(z) - onehot) scale), rows with an
    ignored label exactly 0 (their bound is 0).  p = e / sum: e = __expf(z - m) is off by (|z - m| + 3) 2^-24 of itself (the subtraction's
    rounding and the product with log2 e move the exponent by |z - m| 2^-24 each way at most, v_exp_f32 is good to 2 * 2^-24; line 546), the sum
    by the p-weighted mean of that plus its depth ceil(V / 256) + 6 + 3 (lines 546-547), then 1 / sum, * inv, - 1, * scale (lines 548-553): 4
    more.  The one-hot term enters through the rounding of p - 1 and of the scaling: 2 * 2^-24 |p - onehot|.
    loss = loss0 + sum_r (m + log(sum) - z[label]) scale in fp32 (lines 555, 558-564): each row's three terms pass 4 operations (logf at 2
    roundings) and log(sum) carries the sum's relative error as an absolute one; the ordered sum has depth ceil(n / 256) + 6 + 3 + 1."""
    n, V = z64.shape
    s = f32(scale)
    valid = labels != CE_IGNORE
    lab = labels.clamp_min(0)
    m = z64.max(-1, keepdim=True).values
    d = (z64 - m).abs()
    e = torch.exp(z64 - m)
    tot = e.sum(-1, keepdim=True)
    p = e / tot
    onehot = torch.zeros_like(p).scatter_(1, lab[:, None], 1.0)
    sum_rel = (p * (d + 3.0)).sum(-1, keepdim=True) + (_cdiv(V, 256) + 9)
    vm = valid[:, None].to(z64.dtype)
    dref = (p - onehot) * s * vm
    dacc = abs(s) * (p * (d + 3.0 + sum_rel + 4.0) + 2.0 * (p - onehot).abs()) * vm
    dbound = train_bound(dref, dacc, floor=2 * FTZ) * vm
    zl = z64.gather(1, lab[:, None])
    rows = (m + tot.log() - zl) * s * vm
    loss_ref = f32(loss0) + float(rows.sum())
    mag = abs(f32(loss0)) + float(((m.abs() + tot.log().abs() + zl.abs()) * abs(s) * vm).sum())
    loss_bound = FP32_U * ((_cdiv(n, 256) + 10 + 4) * mag + float((sum_rel * abs(s) * vm).sum()))
    return dref, dbound, dacc, loss_ref, loss_bound


# -- GELU (tanh and erf forms), SwiGLU and their backwards (train.hip:57-149, common.h:53-61) ------------------------------------------------------
GELU_K0, GELU_K1 = f32(0.7978845608028654), f32(0.044715)
ERF_C, PDF_C = f32(0.7071067811865476), f32(0.3989422804014327)
ERF_ULPS = 8.0              # erff is taken as good to 4 ulp = 8 * 2^-24 of its value (the device library's polynomial forms are within a few
                            # ulp); the figure matters only where 1 + erf cancels, below z = -3.5, and is an assumption, not a count
SAT = 20.0                  # 2 e^-20 = 4.2e-9 < 2^-25 = 3.0e-8, with room for E's own error: above it 1.f + __expf(-u) is 1.f exactly and
                            # v_rcp_f32(1.f) = 1.f (a power of two); below -SAT 2 s - 1 rounds to -1.f exactly (half the spacing there is 2^-25)


def _sigmoid_err(u64):
    """s = 1 / (1 + E), E = __expf(-u) -> (s, relative fp32 error of s in units of 2^-24 for a correctly rounded or 1-ulp reciprocal).  E is off by
    (|u| + 2) 2^-24 of itself (silu_f_rel_err's argument), which reaches s times E / (1 + E) = 1 - s; the sum and the reciprocal / division add 6."""
    s = 1.0 / (1.0 + torch.exp(-u64))
    return s, (u64.abs() + 2.0) * (1.0 - s) + 6.0


def _gelu_tanh_u(x64):
    """u2 = 2 k0 (x + k1 x^3) (common.h:57, train.hip:59) and the relative error of its fp32 value in 2^-24: 5 operations, no cancellation."""
    return 2.0 * GELU_K0 * (x64 + GELU_K1 * x64 * x64 * x64), 5.0


def gelu_tanh_fwd_bound(x64):
    """y = bf16(x * rcp(1 + __expf(-u2))) (common.h:53-59).  u2's relative error 5 * 2^-24 is an absolute one of the exponent, 5 |u2| 2^-24, so E is
    off by (6 |u2| + 2) 2^-24 of itself; then as _sigmoid_err, and the product with x."""
    u2, ur = _gelu_tanh_u(x64)
    s = 1.0 / (1.0 + torch.exp(-u2))
    ref = x64 * s
    acc = (((ur + 1.0) * u2.abs() + 2.0) * (1.0 - s) + 7.0) * ref.abs()
    return ref, train_bound(ref, acc, floor=FTZ * (1.0 + x64.abs())), acc


def _one_plus_erf(a64):
    """1 + erf(a) without cancellation in fp64."""
    return torch.where(a64 < 0, torch.special.erfc(-a64), 1.0 + torch.erf(a64))


def gelu_erf_fwd_bound(x64):
    """y = bf16(0.5 x (1 + erff(x c))) (common.h:60).  erff's value is off by ERF_ULPS 2^-24 |erf| and, through its argument's rounding, by
    erf'(a) |a| 2^-24 <= 0.49 * 2^-24; the sum rounds once: 10.5 * 2^-24 (1 + |erf|) at most, an ABSOLUTE error where 1 + erf cancels (x < -4);
    two products follow.  mag = 0.5 |x| (1 + |erf|), 13 roundings."""
    a = x64 * ERF_C
    ref = 0.5 * x64 * _one_plus_erf(a)
    acc = 13.0 * 0.5 * x64.abs() * (1.0 + torch.erf(a).abs())
    return ref, train_bound(ref, acc), acc


def gelu_tanh_bwd_bound(x64, dy64):
    """dz = bf16(dy (A + B)), A = 0.5 (1 + t), B = 0.5 x (1 - t^2) k0 (1 + 3 k1 x^2), t = 2 s - 1, s = rcp(1 + __expf(-u2)) (train.hip:57-61).
    dt = 2 s r_s + 2^-24 |t|; d(1 - t^2) = 2 |t| dt + 2^-24 (t^2 + |1 - t^2|); the other factors of B pass 7 roundings; A, the sum and the product
    with dy 2 each.  Where |u2| >= SAT the fp32 t is exactly +-1 (SAT's comment; 2 s < 2^-25 rounds 2 s - 1 to -1), so 1 - t * t and, at -1, A are
    exactly 0: the error there is the true value of what vanished, not a rounding scaled by C ~ x^3.  The sweep stops at |z| = 2^16; from |z| ~ 5e19 on the factor
    1 + 3 k1 x^2 overflows against 1 - t^2 = 0 (0 * inf): outside the contract (train.hip's comment at dgelu_tanh)."""
    u2, ur = _gelu_tanh_u(x64)
    s = 1.0 / (1.0 + torch.exp(-u2))
    r_s = ((ur + 1.0) * u2.abs() + 2.0) * (1.0 - s) + 6.0
    t = 2.0 * s - 1.0
    one_m_t2 = 4.0 * s * (1.0 - s)
    C = (0.5 * x64 * GELU_K0 * (1.0 + 3.0 * GELU_K1 * x64 * x64)).abs()
    A, B = s, C * one_m_t2 * torch.sign(x64)
    ref = dy64 * (A + B)
    sat = u2.abs() >= SAT
    dt = 2.0 * s * r_s + t.abs()                                        # in units of 2^-24
    d_q = torch.where(sat, one_m_t2 / FP32_U, 2.0 * t.abs() * dt + t * t + one_m_t2)
    d_A = torch.where(sat & (u2 < 0), A / FP32_U, 0.5 * dt + 2.0 * A)
    acc = dy64.abs() * (d_A + C * d_q + 8.0 * B.abs() + 2.0 * (A + B).abs())
    return ref, train_bound(ref, acc, floor=FTZ * (1.0 + x64.abs()) * dy64.abs()), acc


def gelu_erf_bwd_bound(x64, dy64):
    """dz = bf16(dy (0.5 (1 + erff(x c)) + x pdf_c __expf(-0.5 x^2))) (train.hip:62-64).  mag = |dy| (0.5 (1 + |erf|) + |x| pdf(x)).  The first
    term passes 13 roundings (gelu_erf_fwd_bound's 10.5, the sum, the product with dy); the exponent -0.5 x^2 log2 e rounds twice, x^2 * 2^-24 of
    the exponential, v_exp_f32 2, the products, the sum and dy 4: x^2 + 6."""
    a = x64 * ERF_C
    A = 0.5 * _one_plus_erf(a)
    B = x64 * PDF_C * torch.exp(-0.5 * x64 * x64)
    ref = dy64 * (A + B)
    acc = dy64.abs() * (13.0 * 0.5 * (1.0 + torch.erf(a).abs()) + (x64 * x64 + 6.0) * B.abs())
    return ref, train_bound(ref, acc, floor=FTZ * (1.0 + x64.abs()) * dy64.abs()), acc


def silu_mul_fwd_bound(g64, u64):
    """a = bf16(bf16(silu_f(g)) * u), HF's two roundings (train.hip:118) -> (ref, bound, acc, near).  As rmsnorm_fwd_bound: the reference rounds the
    inner value first, the product is exact in fp32, and only an element whose silu(g) lies within silu_f_rel_err(|g|) |silu(g)| of a rounding
    tie may take one inner ulp, |u| ulp, more.  (A flushed denormal intermediate moves the inner value by at most 2^-126, and only where it is
    itself below 2^-118, where an inner ulp is below 2^-126: the floor FTZ (1 + |g|) (1 + |u|) carries both.)"""
    inner = g64 / (1.0 + torch.exp(-g64))
    near, ulp = bf16_near_tie(inner, silu_f_rel_err(g64.abs()) * inner.abs())
    ref = bf16_round64(inner) * u64
    acc = torch.where(near, u64.abs() * ulp / FP32_U, torch.zeros_like(ref))
    return ref, train_bound(ref, acc, floor=FTZ * (1.0 + g64.abs()) * (1.0 + u64.abs())), acc, near


def silu_mul_bwd_bound(g64, u64, da64):
    """dg = bf16(da u dsilu(g)), du = bf16(da silu_f(g)) (train.hip:122-137) -> ((dg ref, bound, acc), (du ref, bound, acc)).
    dsilu = s (1 + x (1 - s)), s = 1.f / (1.f + __expf(-x)): ds = s r_s; d(1 - s) = ds + 2^-24 (1 - s); d(x (1 - s)) = |x| d(1 - s) + 2^-24 |x (1 - s)|;
    the sum and the last product round once each.  Where x >= SAT the fp32 s is exactly 1 (SAT's comment) and 1 - s exactly 0: there
    ds = d(1 - s) = 1 - s, the true value of what vanished.  da * u is exact in fp32; its product with dsilu rounds once.
    du: silu_f_rel_err and the product."""
    x = g64
    s, r_s = _sigmoid_err(x)
    sat = x >= SAT
    ds = torch.where(sat, (1.0 - s) / FP32_U, s * r_s)                   # units of 2^-24
    d1s = torch.where(sat, (1.0 - s) / FP32_U, ds + (1.0 - s))
    inner = 1.0 + x * (1.0 - s)
    d_inner = x.abs() * d1s + (x * (1.0 - s)).abs() + inner.abs()
    dsilu = s * inner
    d_dsilu = ds * inner.abs() + s * d_inner + dsilu.abs()
    dg = da64 * u64 * dsilu
    acc_g = (da64 * u64).abs() * (d_dsilu + dsilu.abs())
    floor = FTZ * (1.0 + x.abs())
    silu = x * s
    du = da64 * silu
    acc_u = (silu_f_rel_err(x.abs()) / FP32_U + 1.0) * du.abs()
    return (dg, train_bound(dg, acc_g, floor=floor * (1.0 + x.abs()) * (da64 * u64).abs() + FTZ), acc_g), \
           (du, train_bound(du, acc_u, floor=floor * da64.abs() + FTZ), acc_u)


# -- AdamW (train.hip:678-800) ---------------------------------------------------------------------------------------------------------------------
def adamw_bounds(p64, m64, v64, g64, lr, b1, b2, eps, wd, step: int, grad_scale: float):
    """fp64 AdamW on the C float arguments, the bias corrections formed in fp64 -> {"master" / "m" / "v": (ref, bound)} (fp32 outputs: no bf16
    rounding; param is bf16(master) and compared bit for bit by the caller).  adamw_one (train.hip:678-684):
      g = bf16 grad * grad_scale: 1 rounding.  m' = b1 m + (1 - b1) g: 4 on |b1 m| + |(1 - b1) g| (1.f - b1 is exact for b1 in [0.5, 1)).
      v' = b2 v + (1 - b2) g^2: 5 (g enters twice).  p1 = p (1 - lr wd): 3 on |p|.
      bc = 1 - powf(b, step) on the host (train.hip:719): powf within 1 ulp = 2 * 2^-24 of b^step, the subtraction rounds once: (2 b^step / bc + 1) 2^-24
      of bc, a large relative error at step 1 and 2 of b2 = 0.999 that the bound has to carry.
      den = sqrtf(v' / bc2) + eps: sqrt halves the relative error of its argument (dv / v' + bc2's + the division), sqrtf and the sum round once each.
      upd = lr (m' / bc1) / den: m's absolute error scaled by lr / (bc1 den), and |upd| times (bc1's + den's relative error + 4).
      p' = p1 - upd rounds at |p'|."""
    lr, b1, b2, eps, wd, gs = (f32(a) for a in (lr, b1, b2, eps, wd, grad_scale))
    g = g64 * gs
    m1a, m1b = b1 * m64, (1.0 - b1) * g
    v1a, v1b = b2 * v64, (1.0 - b2) * g * g
    m1, v1 = m1a + m1b, v1a + v1b
    dm = 4.0 * (m1a.abs() + m1b.abs())                                  # units of 2^-24
    dv = 5.0 * (v1a.abs() + v1b.abs())
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    r_bc1, r_bc2 = 2.0 * b1 ** step / bc1 + 1.0, 2.0 * b2 ** step / bc2 + 1.0
    root = (v1 / bc2).sqrt()
    den = root + eps
    d_den = root * (0.5 * (dv / v1.clamp_min(1e-300) + r_bc2 + 1.0) + 1.0) + den
    upd = lr * (m1 / bc1) / den
    d_upd = lr / (bc1 * den) * dm + upd.abs() * (r_bc1 + d_den / den + 4.0)
    p1 = p64 * (1.0 - lr * wd)
    pn = p1 - upd
    d_p = 3.0 * p64.abs() + d_upd + pn.abs()
    return {"master": (pn, train_bound(pn, d_p, roundings=0, floor=FTZ)), "m": (m1, train_bound(m1, dm, roundings=0, floor=FTZ)),
            "v": (v1, train_bound(v1, dv, roundings=0, floor=FTZ))}


# -- scatter_add_rows and depth_to_space: exact references ---------------------------------------------------------------------------------------
def scatter_add_rows_ref(src: torch.Tensor, dst: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """The documented order (train.hip:576-611): for every id its first occurrence, the later occurrences added in ascending order in fp32, then
    old + sum rounded once.  -> the new table (dst is not modified)."""
    out = dst.clone()
    order = {}
    for i, r in enumerate(ids.tolist()):
        order.setdefault(int(r), []).append(i)
    for r, occ in order.items():
        a = src[occ[0]].float()
        for j in occ[1:]:
            a = a + src[j].float()
        out[r] = (dst[r].float() + a).to(torch.bfloat16)
    return out


def depth_to_space_index_map(B: int, g: int, k: int) -> torch.Tensor:
    """[B, g * g] int64: for every source cell (b, sy, sx) the flat index into dy viewed as [B * gd * gd * k * k] cells of C channels, obtained
    by sending the cell numbers 1 .. through oracle.vila_oracle.downsample_block (0 marks its zero padding)."""
    from oracle.vila_oracle import downsample_block
    idx = torch.arange(1, B * g * g + 1, dtype=torch.float64).reshape(B, g * g, 1)
    y = downsample_block(idx, k).reshape(-1).long()                      # [B * gd * gd * k * k]: the source cell (+1) each dy cell came from
    pos = torch.full((B * g * g + 1,), -1, dtype=torch.int64)
    pos[y] = torch.arange(y.numel())
    assert bool((pos[1:] >= 0).all())
    return pos[1:].reshape(B, g * g)


# ---- the W4A16 kernels (vila_amd/csrc/gemv_w4.hip, gemv_w4_batch.hip, gemm_w4.hip): exact cases, exact references and a per-element bound ------
# (tests/test_w4_bound_cpu.py proves them, tests/test_gpu_w4_elements.py uses them).  The kernels never dequantise: per 128-wide group they sum
# x (128 + q) on the matrix cores, remove (128 + zero) sum(x) in fp32 and add scale * that to a running total with one fmaf.  With integer
# activations and power-of-two scales every one of those values is an integer multiple of 2^kmin below 2^24 of them: each operation is exact, the
# fp32 value before the epilogue equals the fp64 product whatever the order of groups, waves, tiles or K-slices, and a plain output is the bf16
# rounding of that product BIT FOR BIT.  Ordinary inputs get a bound derived from what the kernels add (w4_generic_acc).
def exact_w4(shape, seed, log2_scale=(-7, -6, -5), device="cpu"):
    """Weights exactly representable as (q - zero) * 2^k with every group spanning q = 0..15.  device "cuda": drawn there (other numbers, the same
    construction), for matrices of 10^8 weights."""
    N, K = shape
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randint(0, 16, (N, K // 128, 128), generator=g, device=device)
    q[..., 0], q[..., 1] = 0, 15
    zero = torch.randint(4, 12, (N, K // 128, 1), generator=g, device=device)
    k = torch.tensor(log2_scale, device=device)[torch.randint(0, len(log2_scale), (N, K // 128, 1), generator=g, device=device)]
    return ((q - zero).float() * torch.exp2(k.float())).view(N, K)


W4_EXACT_QZ = 11            # max |q - zero| of exact_w4: q in 0..15, zero in 4..11
W4_EXACT_ADDEND = 64        # bias and residual of an exact case: integers up to this, times 2^kmin (the residual times res_mult as well)


def w4_exact_case(N: int, K: int, seed: int, log2_scales=(-7, -6, -5), x_max: int = 4, rows: int = 16, gateup: bool = False, heads=None,
                  normed: bool = False, x_pow: int = 1, device="cpu") -> dict:
    """One problem of the exact regime -> dict:
      w [N, K] fp32 (gateup: w = gate, w_up = up), exact_w4 weights; mat: their W4Matrix on `device` (heads = (q, kv, head_dim): packed with
      quant.rope_interleave_rows, N = (q + 2 kv) head_dim), quantise -> dequantise asserted to be the identity;
      x [rows, K] bf16: integers in [-x_max, x_max]; x_eff: what the kernel multiplies (x itself);
      bias [N], res [rows, N] bf16: integers up to 64 times 2^kmin (the residual also times res_mult, the power of two next below sqrt(K / 128), so
      that it stays of the size of the projection's own bf16 spacing at every K and the order of the two roundings of the residual epilogue shows);
      core [rows, N] fp64 = x_eff . w^T (core_up with gateup), exact: every term is an integer multiple of 2^kmin.
    normed (the fused RMSNorm of stage_x_w4, gemv_w4.hip:63-71): every |x_k| = 2^x_pow with random signs, norm_w integers in [-x_max, x_max]
    (zeros included), eps = 1e-6.  Then sum x^2 = K 4^x_pow and its mean 4^x_pow are exact in fp32 in any order, rstd = rsqrtf(4^x_pow + 1e-6) is
    2^-x_pow (1 - 5e-7 / 4^x_pow) up to a few ulp, x rstd = +-(1 - 5e-7 ..): 2^-9 away from the nearest bf16 rounding tie, so bfround(x rstd) is +-1
    whatever the last ulp of rsqrtf or of the division, and the staged value bfround(norm_w * +-1) = +-norm_w.  x_eff holds those (x_pow >= 0: with
    |x| << 1e-3 the eps would dominate).
    Asserted here: the worst partial sum G 128 x_max 11 2^(kmax - kmin) plus bias and residual stays below 2^24 in units of 2^kmin, so every
    intermediate (a group's sum of x (128 + q) < 128 x_max 143 < 2^17, (128 + zero) sum x <= 139 * 128 x_max, their integer difference, the fmaf
    with a power-of-two scale, the wave and slab partials, bias, bfround(v) + residual) is exact in fp32."""
    from vila_amd.quant import W4Matrix, rope_interleave_rows
    kmin, kmax = min(log2_scales), max(log2_scales)
    G, u = K // 128, 2.0 ** min(log2_scales)
    if heads is not None:
        nq, nkv, hd = heads
        assert N == (nq + 2 * nkv) * hd and not gateup
    g = torch.Generator().manual_seed(seed + 12345)
    res_mult = 1
    while 4 * res_mult * res_mult <= G:
        res_mult *= 2
    worst = G * 128 * x_max * W4_EXACT_QZ * 2 ** (kmax - kmin) + W4_EXACT_ADDEND * (1 + res_mult)
    assert worst < 2 ** 24 and x_pow >= 0, (N, K, log2_scales, x_max, worst)
    c = {"N": N, "K": K, "u": u, "gateup": gateup, "heads": heads, "eps": 1e-6}
    wdev = device if N * K >= 1 << 24 else "cpu"             # (matrices of 10^7 weights and more are drawn where they are used)
    c["w"] = exact_w4((N, K), seed, log2_scales, wdev)
    if gateup:
        c["w_up"] = exact_w4((N, K), seed + 1, log2_scales, wdev)
    if normed:
        c["x"] = ((torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).float() * 2.0 ** x_pow).to(torch.bfloat16)
        c["norm_w"] = torch.randint(-x_max, x_max + 1, (K,), generator=g).to(torch.bfloat16)
        c["x_eff"] = (torch.sign(c["x"].float()) * c["norm_w"].float()).to(torch.bfloat16)
    else:
        c["x"] = torch.randint(-x_max, x_max + 1, (rows, K), generator=g).to(torch.bfloat16)
        c["norm_w"], c["x_eff"] = None, c["x"]
    c["bias"] = (torch.randint(-W4_EXACT_ADDEND, W4_EXACT_ADDEND + 1, (N,), generator=g).float() * u).to(torch.bfloat16)
    c["res"] = (torch.randint(-W4_EXACT_ADDEND, W4_EXACT_ADDEND + 1, (rows, N), generator=g).float() * (u * res_mult)).to(torch.bfloat16)
    assert float(c["bias"].float().abs().max()) <= W4_EXACT_ADDEND * u and float(c["res"].float().abs().max()) <= W4_EXACT_ADDEND * u * res_mult
    dev = torch.device(device)
    for k in ("w", "w_up", "x", "x_eff", "norm_w", "bias", "res"):
        if c.get(k) is not None:
            c[k] = c[k].to(dev)
    perm = rope_interleave_rows(nq + nkv, nq + 2 * nkv, hd, device=dev) if heads is not None else None
    c["mat"] = W4Matrix.pack(c["w"], c.get("w_up"), row_perm=perm)
    d = c["mat"].dequantized()
    for got, want in zip(d if gateup else (d,), (c["w"], c.get("w_up"))):
        assert torch.equal(got, want), f"quantise -> dequantise of the exact weights ({N}, {K}) is not the identity"
    xe = c["x_eff"].double()
    c["core"] = xe @ c["w"].double().t()
    if gateup:
        c["core_up"] = xe @ c["w_up"].double().t()
    assert float(c["core"].abs().max()) / u + W4_EXACT_ADDEND * (1 + res_mult) < 2 ** 24
    return c


def w4_exact_plain_ref(core64: torch.Tensor, bias64=None, res64=None) -> torch.Tensor:
    """The bf16 result of a plain epilogue in the exact regime, to be compared as bits.  v = sum + bias is exact; without a residual the output is
    its bf16 rounding; with one the kernels round twice, f2bf(bfround(v) + r) (gemv_w4.hip:233-235, gemv_w4_batch.hip:118-120, gemm_w4.hip:67-69),
    and bfround(v) + r is exact in fp32 too (both are multiples of 2^kmin below 2^24 of them)."""
    v = core64 if bias64 is None else core64 + bias64
    if res64 is None:
        return v.to(torch.bfloat16)
    return (bf16_round64(v) + res64).to(torch.bfloat16)


def assert_bits_equal(out: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """out and ref, bf16 [rows, cols], identical bit for bit; a failure states the count and the (row, col, got, expected) of the first few."""
    assert out.shape == ref.shape and out.dtype == ref.dtype == torch.bfloat16, (tuple(out.shape), tuple(ref.shape), out.dtype, ref.dtype)
    o, r = out.contiguous().view(torch.int16), ref.to(out.device).contiguous().view(torch.int16)
    bad = o != r
    k = int(bad.sum())
    if k:
        o2, r2 = out.reshape(-1, out.shape[-1]), ref.to(out.device).reshape(-1, out.shape[-1])
        at = [(int(i), int(j), float(o2[i, j]), float(r2[i, j])) for i, j in bad.reshape(o2.shape).nonzero()[:8].tolist()]
        raise AssertionError(f"{what}: {k} of {out.numel()} elements differ from the exact result; first (row, col, got, expected) {at}")


def w4_unpack(logical):
    """quant.py's logical arrays -> (q [N, K], zero [N, G], scale [N, G]) in fp64: the integers and the bf16 scales the kernels read."""
    wq, wsz = logical
    N, K8 = wq.shape
    q = torch.empty((N, K8, 8), dtype=torch.float64, device=wq.device)
    for p in range(4):
        q[..., 2 * p] = ((wq >> (4 * p)) & 0xF).double()
        q[..., 2 * p + 1] = ((wq >> (4 * (p + 4))) & 0xF).double()
    scale = (wsz & 0xFFFF).to(torch.int16).view(torch.bfloat16).double()
    zero = ((wsz >> 16) & 0xFFFF).to(torch.int16).view(torch.bfloat16).double() - 128.0
    return q.view(N, K8 * 8), zero, scale


W4_SUM_OPS = 129            # roundings one product of a group passes at most: 128 additions of an fp32 sum in any order (the four MFMAs of a group
                            # add 32 products each to an accumulator, two chains, gemv_w4.hip:208-218, gemv_w4_batch.hip:76-86, gemm_w4.hip:143-155)
                            # and the addition of the two chains (gemv_w4.hip:219).  The group sum of x passes at most 128 too (an MFMA against ones in
                            # gemv_w4_batch.hip:78; three tree levels and four shuffles, 7, in gemv_w4.hip:77-84 and gemm_w4.hip:103-106) and the
                            # product with 128 + zero one more (gemv_w4.hip:219, gemv_w4_batch.hip:92, gemm_w4.hip:165)
W4_CHAIN_EXTRA = 20         # roundings behind a group's difference D - zp S besides the G fmaf of the chain: the subtraction itself, the <= 16 wave
                            # partials (gemv_w4.hip:229, gemv_w4_batch.hip:110-114) or <= 8 slabs (gemm_w4.hip:201), the bias, and the fp32 addition of
                            # the residual


W4_NORM_DEPTH = 60          # fp32 roundings behind x rstd in stage_x_w4 (gemv_w4.hip:44-71): a thread adds at most 4 chunks of 8 squares, 6 shuffle levels,
                            # the <= 16 wave sums, / K, + eps, rsqrtf (2), the product; half of the sum's relative error reaches rstd, the bound takes all


def w4_staged_norm(x64: torch.Tensor, norm_w64: torch.Tensor, eps: float):
    """The activation stage_x_w4 leaves in LDS with a fused RMSNorm, bfround(w * bfround(x rstd)) (gemv_w4.hip:70-71) -> (x_eff bf16, slack fp64).
    As rmsnorm_fwd_bound: an element whose x rstd lies within the fp32 error of a bf16 rounding tie may come out one inner ulp away, which moves
    the staged value by at most |w| ulp and then by one bf16 spacing of the product; slack holds that (0 elsewhere), for w4_generic_acc."""
    _, _, inner = norm_stats64(x64, True, eps)
    near, ulp = bf16_near_tie(inner, W4_NORM_DEPTH * FP32_U * inner.abs())
    staged = norm_w64 * bf16_round64(inner)
    slack = torch.where(near, norm_w64.abs() * ulp + 2 * BF16_U * staged.abs(), torch.zeros_like(staged))
    return staged.to(torch.bfloat16), slack


def w4_generic_acc(x64: torch.Tensor, q64: torch.Tensor, zero64: torch.Tensor, scale64: torch.Tensor, x_slack64: torch.Tensor = None):
    """-> (core [n, N], acc [n, N]) in fp64 for x64 [n, K] and unpacked weights [N, K] / [N, G]: core = x . ((q - zero) scale)^T, the product with
    the dequantised weights, and acc, the first-order bound on the fp32 error of the kernels' sum before the epilogue,
        2^-24 [ 129 sum_g s_g (sum_k |x_k| (128 + q_k) + zp_g sum_k |x_k|)  +  (G + 20) sum_g s_g sum_k |x_k| |q_k - z_g| ],   zp = 128 + zero.
    Per group: D = the fp32 sum of 128 exact products x (128 + q) (bf16 x bf16 is exact in fp32) in any order, off by 129 * 2^-24 of the sum of
    their magnitudes; P = zp S with S the group sum of x, off by (128 + 1) 2^-24 zp sum |x|; the subtraction D - P rounds once, at the size of the
    true difference sum x (q - z) (first order), which sum |x| |q - z| bounds; so does every later operation the difference passes, each scaled by
    s: the fmaf of its own and of the later groups of the chain (<= G), the partials, the bias, the residual (W4_CHAIN_EXTRA).  The first term is
    the price of never dequantising: it is of the size of K 2^-24 * 129 * 135 |x| s, where a dequantising kernel would pay K 2^-24 |x| |w|.
    x_slack64 [n, K] (w4_staged_norm): by how much a staged activation may differ from x64; acc gains x_slack . |w|^T."""
    N, K = q64.shape
    G = K // 128
    n = x64.shape[0]
    xa = x64.abs()
    sk = scale64.repeat_interleave(128, 1)
    zk = zero64.repeat_interleave(128, 1)
    core = x64 @ ((q64 - zk) * sk).t()
    t1 = xa @ ((128.0 + q64) * sk).t()
    t2 = xa.view(n, G, 128).sum(-1) @ ((128.0 + zero64) * scale64).t()
    t3 = xa @ ((q64 - zk).abs() * sk).t()
    acc = FP32_U * (W4_SUM_OPS * (t1 + t2) + (G + W4_CHAIN_EXTRA) * t3)
    if x_slack64 is not None:
        acc = acc + x_slack64 @ ((q64 - zk).abs() * sk).t()
    return core, acc


def w4_absprod(acc64: torch.Tensor, K: int) -> torch.Tensor:
    """The `absprod` argument with which bgemm_acc_bound(., K) gives (1 + 2^-8) acc: the W4 kernels' epilogues round as bgemm_epilogue does
    (gemv_w4_batch.hip's header), so bgemm_plain_bound / bgemm_gateup_bound / bgemm_qkv_bound supply the rounding terms and this the accumulation
    term.  acc = 0 (the exact regime): the epilogue's own roundings and silu_f's error alone."""
    return acc64 / ((K + BGEMM_EXTRA_OPS) * FP32_U)


def w4_generic_bound(kind: str, K: int, core64, acc64, core_up64=None, acc_up64=None, bias64=None, res64=None, cs64=None, heads=None):
    """-> (ref, bound) per element for ordinary inputs.  kind "plain" (modes 0 and 4, and the prefill's q|k|v form, which adds the bias and stores in
    natural order without RoPE), "gateup", "qkv" (bias + RoPE; ref in natural q | k | v column order).  The bgemm bounds add |bias| and |residual|
    to absprod, (K + 10) 2^-24 of them: more than the one rounding each really costs, and below 1e-5 of either."""
    if kind == "plain":
        return bgemm_plain_bound(core64, w4_absprod(acc64, K), K, bias64, res64)
    if kind == "gateup":
        return bgemm_gateup_bound(core64, w4_absprod(acc64, K), core_up64, w4_absprod(acc_up64, K), K)
    assert kind == "qkv"
    return bgemm_qkv_bound(core64, w4_absprod(acc64, K), K, bias64, cs64, *heads)


# ---- the prefill / SFT attention (vila_amd/csrc/attn.hip, attn_bwd.hip, attn_bwd_dma.hip): per-element references and bounds ------------------------
# (tests/test_attn_bound_cpu.py proves them, tests/test_gpu_attn_elements.py uses them).  Everything is computed in fp64 per sequence and kv head,
# as attn_ref does; the bounds have train_bound's shape with one more rounding term, 2^-8 of the magnitudes that pass a bf16 operand (P or t).
# Notation: x = s * scale the scaled score of a (row, key) pair (scale as the C float), M the row's maximum of x over its visible keys, p the exact
# softmax weights, u = 2^-24.  All "units of u" below are counts of fp32 roundings read from the cited lines.
ATTN_KT = 64                # keys per K / V tile (attn.hip:26, attn_common.h AttnDma::KT); also the key block of both dK / dV kernels
ATTN_EXP_OPS = 3            # one rescale of a running sum: v_exp_f32 (1 ulp = 2 u) and the product with it (attn.hip:555, 575, 580; 651-658)
ATTN_DELTA_DEPTH = 12       # attn_bwd.hip:30-32: a lane adds its 8 products (exact: bf16 x bf16) one after the other, then 4 shuffle levels


def _attn_blocks(T: int, Hkv: int, cu):
    bounds = [0, T] if cu is None else [int(b) for b in cu.tolist()]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b > a:
            for g in range(Hkv):
                yield a, b, g


def attn_visible(Lq: int, Lk: int, causal: bool, past: int = 0, device="cpu") -> torch.Tensor:
    """[Lq, Lk] bool: row i sees key j iff j <= past + i (causal), every key otherwise."""
    if not causal:
        return torch.ones((Lq, Lk), dtype=torch.bool, device=device)
    return torch.arange(Lk, device=device)[None, :] <= past + torch.arange(Lq, device=device)[:, None]


def _attn_scores(q, k, a, b, g, G, s, causal, past):
    """One (sequence, kv head) block -> q64 [G, L, D], k64 [Lk, D], vis [L, Lk], x [G, L, Lk] (masked: -inf), A = scale |q| . |k|."""
    ka, kb = (0, k.shape[0]) if past else (a, b)
    q64 = q[a:b, g * G:(g + 1) * G].double().transpose(0, 1)
    k64 = k[ka:kb, g].double()
    vis = attn_visible(b - a, kb - ka, causal, past, q.device)
    x = torch.einsum("hqd,kd->hqk", q64, k64) * s
    A = torch.einsum("hqd,kd->hqk", q64.abs(), k64.abs()) * abs(s)
    return q64, k64, vis, x.masked_fill(~vis, float("-inf")), A


def attn_fwd_bounds(q, k, v, causal: bool, cu=None, scale=None, past: int = 0) -> dict:
    """q [T, Hq, D], k / v [Tk, Hkv, D] bf16 (Tk = T; with `past`, ONE sequence whose Tk = past + T keys start `past` positions before its
    queries: the append prefill) -> {"o": (ref, bound, acc) [T, Hq, D], "lse": (ref, bound, acc) [Hq, T], "rnd_o": the rounding part of o's bound}.

    What the kernels do (attn.hip:543-591 and 663-681, the DMA-ring kernel of forms A - D; 160-245 the round-2 kernel, form v1; the same arithmetic):
    the score is an fp32 MFMA sum of D exact products; per 64-key tile e = v_exp_f32(fma(s, c, -m c)) with c = scale * log2 e and m the running
    maximum (line 571), l = l alpha + sum e of the UNROUNDED e (573-575), O = O alpha + V^T bf16(e) (580, 585-588, 620); the key-split forms merge
    two (m, l, O) with a_i = v_exp_f32((m_i - m) c) (650-658); o = bf16(O * (1 / l)) (668, 675), lse = m scale + logf(l) (681).

    The weight a key ends with is e times every later rescale.  In the exponent the chain telescopes to (s - m_final) c, so m's own error drops
    out of o and of lse, and what remains, as a relative error of the weight in units of u, is
        r = (D + 2) A                the score: an fp32 sum of D products in any order, scaled (gemm_elem_bound's term)
          + 5 |x - M|                c's two roundings act on (s - m) c, the fma rounds once at |s c - m c| <= that, and the rescales' exponents
                                     (m_old - m_new) c round twice each and add up to at most (M - x) (m only grows)
          + max |x|                  m c is rounded before the fma (line 562): |m c| u with |m| <= the largest |x| of the row
          + 3 (tiles + 2)            ATTN_EXP_OPS per rescale: one per tile, the merge, and e itself (ce_bounds' "+ 3")
    l: the weights' own errors, p-weighted (rbar), and an fp32 sum of the row's visible keys in any order plus one product per tile and the merge.
    O: bf16(e) is off by 2^-8 e (the rounding term 2^-8 sum p |v|); the fp32 part is r per key, the depth of the PV sum (visible keys), a product per
    tile and the merge; then 1 / l (rbar, l's depth, 5 for a fast reciprocal as silu_f_rel_err counts it) and the product: together
        acc_o = sum_k p_k r_k |v_kd| + sum_k p_k |v_kd| (rbar + 2 (visible + tiles) + 11).
    lse = m scale + logf(l): rbar and l's depth as an absolute error, |M| for the product m scale, logf at 2 ulp of |log l|, the sum at |lse|.
    Floor: v_exp_f32 and the bf16 conversion flush below 2^-126, per key at most FTZ |v|."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    s = f32(D ** -0.5 if scale is None else scale)
    dev = q.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    ref, rnd, acc, floor = z(T, Hq, D), z(T, Hq, D), z(T, Hq, D), z(T, Hq, D)
    lref, lacc = z(Hq, T), z(Hq, T)
    assert not (past and cu is not None)
    for a, b, g in _attn_blocks(T, Hkv, cu):
        hs = slice(g * G, (g + 1) * G)
        _, _, vis, x, A = _attn_scores(q, k, a, b, g, G, s, causal, past)
        v64 = v[(slice(None) if past else slice(a, b)), g].double()
        M = x.max(-1, keepdim=True).values
        e = torch.exp(x - M)
        l = e.sum(-1, keepdim=True)
        p = e / l
        nvis = vis.sum(-1).double()                                     # [L]
        tiles = torch.ceil(nvis / ATTN_KT)
        r = (D + 2) * A + 5.0 * torch.where(vis, M - x, torch.zeros_like(x)) + torch.where(vis, x.abs(), torch.zeros_like(x)).max(-1, keepdim=True).values \
            + ATTN_EXP_OPS * (tiles[None, :, None] + 2.0)
        rbar = (p * r).sum(-1)                                          # [G, L]
        depth = nvis + tiles
        av = v64.abs()
        S1 = torch.einsum("hqk,kd->hqd", p, av)
        ref[a:b, hs] = torch.einsum("hqk,kd->hqd", p, v64).transpose(0, 1)
        rnd[a:b, hs] = S1.transpose(0, 1)
        acc[a:b, hs] = (torch.einsum("hqk,kd->hqd", p * r, av) + S1 * (rbar + 2.0 * depth[None, :] + 11.0)[..., None]).transpose(0, 1)
        floor[a:b, hs] = FTZ * (1.0 + av.sum(0))
        lse = (M + l.log())[..., 0]
        lref[hs, a:b] = lse
        lacc[hs, a:b] = rbar + depth[None, :] + 3.0 + M[..., 0].abs() + 4.0 * l.log()[..., 0].abs() + lse.abs() + 2.0
    rnd_o = BF16_U * ref.abs() + BF16_U * rnd
    bound = BF16_U * ref.abs() + (1.0 + BF16_U) * (BF16_U * rnd + FP32_U * acc) + floor
    return {"o": (ref, bound, acc), "lse": (lref, train_bound(lref, lacc, roundings=0), lacc), "rnd_o": rnd_o}


def attn_bwd_bounds(q, k, v, do, o, lse, causal: bool, cu=None, scale=None, o_err=None, lse_err=None) -> dict:
    """The backward operator on ITS inputs: o [T, Hq, D] and lse [Hq, T] are what it consumes (ops.attn_bwd) -> {"delta" / "dq" / "dk" / "dv":
    (ref, bound, acc), "rnd_dq" / "rnd_dk" / "rnd_dv": the rounding parts}.  References in fp64:
        P = exp(x - lse),  delta = sum_d o do,  dP = do . V^T,  t = P (dP - delta) scale,  dv = P^T do,  dq = t K,  dk = t^T Q
    (dk and dv summed over the query rows and the G heads of the group).  The kernels (attn_bwd_dma.hip:174-191, 398-402, 446-448; attn_bwd.hip:19-34,
    159-179, 366-379 and the pack2bf stores) round P to bf16 before dV, t to bf16 before dQ and dK, and every output once.
    delta (attn_bwd.hip:30-33): ATTN_DELTA_DEPTH u sum_d |o do|, an fp32 output.
    P = v_exp_f32(fma(s, c, -lse log2 e)): relative error in units of u
        rP = (D + 1) A + 3 |x| + 2 |lse| + |x - lse| + 2
    (the score; c's two roundings and, without fma contraction in attn_bwd.hip:169, the product's; lse * LOG2E: the constant and the product; the
    subtraction; the exponential).  dP is an fp32 sum of D products, (D + 1) u B with B = |do| . |v|^T; dP - delta rounds once and carries delta's
    error; two products follow.  So t is off, before its bf16 rounding, by the CARRIED error
        dt = |t| (rP + 3) + P scale ((D + 1) B + ATTN_DELTA_DEPTH sum_d |o do|)      (units of u)
    whose second part does not shrink where dP - delta cancels: with P near 1 (large logits) t vanishes and dt does not.
        dv: 2^-8 |ref| + (1 + 2^-8) [2^-8 sum P |do| + u (sum P rP |do| + (n + 2) sum P |do|)]
        dq: 2^-8 |ref| + (1 + 2^-8) [2^-8 sum_k |t| |K| + u (sum_k dt |K| + (visible + 1) sum_k |t| |K|)]
        dk: as dq over the n = G * (rows that see the key) terms, + 2 for the two halves that meet in LDS (attn_bwd.hip:413-418, attn_bwd_dma.hip:433-438).
    o_err / lse_err (end to end: o and lse come from the project's forward, the reference uses the exact ones): the forward's own bounds, carried
    through delta (sum_d o_err |do|) and P (lse_err, relative)."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    s = f32(D ** -0.5 if scale is None else scale)
    dev = q.device
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    out = {n: [z(T, h, D) for _ in range(4)] for n, h in (("dq", Hq), ("dk", Hkv), ("dv", Hkv))}       # ref, rnd, acc, floor
    dref, dacc = z(Hq, T), z(Hq, T)
    for a, b, g in _attn_blocks(T, Hkv, cu):
        hs = slice(g * G, (g + 1) * G)
        q64, k64, vis, x, A = _attn_scores(q, k, a, b, g, G, s, causal, 0)
        v64 = v[a:b, g].double()
        do64 = do[a:b, hs].double().transpose(0, 1)
        o64 = o[a:b, hs].double().transpose(0, 1)
        lse64 = lse[hs, a:b].double()[..., None]
        P = torch.exp(x - lse64)                                        # masked: exp(-inf) = 0
        x0 = torch.where(vis, x, torch.zeros_like(x))
        delta = (o64 * do64).sum(-1)
        Dd = ATTN_DELTA_DEPTH * (o64 * do64).abs().sum(-1)
        dref[hs, a:b], dacc[hs, a:b] = delta, Dd
        if o_err is not None:
            Dd = Dd + (o_err[a:b, hs].double().transpose(0, 1) * do64.abs()).sum(-1) / FP32_U
        diff = torch.einsum("hqd,kd->hqk", do64, v64) - delta[..., None]
        B = torch.einsum("hqd,kd->hqk", do64.abs(), v64.abs())
        t = P * diff * s
        rP = (D + 1) * A + 3.0 * x0.abs() + 2.0 * lse64.abs() + torch.where(vis, (x0 - lse64).abs(), torch.zeros_like(x0)) + 2.0
        if lse_err is not None:
            rP = rP + lse_err[hs, a:b].double()[..., None] / FP32_U
        dt = t.abs() * (rP + 3.0) + P * abs(s) * ((D + 1) * B + Dd[..., None])
        nvis = vis.sum(-1).double()
        nq = G * vis.sum(0).double()
        dmax = 1.0 + abs(s) * float(diff.abs().max())
        ka, qa, da = k64.abs(), q64.abs(), do64.abs()
        ref_, rnd_, acc_, fl_ = out["dq"]
        Tq = torch.einsum("hqk,kd->hqd", t.abs(), ka)
        ref_[a:b, hs] = torch.einsum("hqk,kd->hqd", t, k64).transpose(0, 1)
        rnd_[a:b, hs] = Tq.transpose(0, 1)
        acc_[a:b, hs] = (torch.einsum("hqk,kd->hqd", dt, ka) + (nvis + 1.0)[None, :, None] * Tq).transpose(0, 1)
        fl_[a:b, hs] = FTZ * dmax * (1.0 + ka.sum(0))
        ref_, rnd_, acc_, fl_ = out["dk"]
        Tk = torch.einsum("hqk,hqd->kd", t.abs(), qa)
        ref_[a:b, g] = torch.einsum("hqk,hqd->kd", t, q64)
        rnd_[a:b, g] = Tk
        acc_[a:b, g] = torch.einsum("hqk,hqd->kd", dt, qa) + (nq + 2.0)[:, None] * Tk
        fl_[a:b, g] = FTZ * dmax * (1.0 + qa.sum((0, 1)))
        ref_, rnd_, acc_, fl_ = out["dv"]
        Tv = torch.einsum("hqk,hqd->kd", P, da)
        ref_[a:b, g] = torch.einsum("hqk,hqd->kd", P, do64)
        rnd_[a:b, g] = Tv
        acc_[a:b, g] = torch.einsum("hqk,hqd->kd", P * rP, da) + (nq + 2.0)[:, None] * Tv
        fl_[a:b, g] = FTZ * (1.0 + da.sum((0, 1)))
    res = {"delta": (dref, train_bound(dref, dacc, roundings=0), dacc)}
    for n, (ref_, rnd_, acc_, fl_) in out.items():
        res[n] = (ref_, BF16_U * ref_.abs() + (1.0 + BF16_U) * (BF16_U * rnd_ + FP32_U * acc_) + fl_, acc_)
        res["rnd_" + n] = BF16_U * ref_.abs() + BF16_U * rnd_
    return res


def plant_pairs(q: torch.Tensor, k: torch.Tensor, pairs, causal: bool, cu=None, scale=None, weight: float = 0.5, past: int = 0) -> torch.Tensor:
    """Planted pairs for prefill shapes, in place: for every (row, key) of `pairs` (token indices of q and of k; the rows distinct, the keys distinct,
    each pair inside one sequence and visible) and every kv head h, k[key, h] = bf16(alpha q[row, target head of h]) (probe_targets) with alpha
    such that, by the fp64 softmax over the row's visible keys, the planted key carries `weight` of the target head's row: alpha |q|^2 scale =
    log(weight / (1 - weight) * sum of the other keys' exp(x)).  At about 1/2 the pair carries O(|v|) in o, O(|do|) in dv and, unlike a weight of
    about 1, where t = P (dP - delta) vanishes, O(1) in dq and dk.  Two passes: the second sees every other planted key in place.
    -> the weights reached [pairs, Hkv] fp64, which the caller asserts to lie in 0.3 .. 0.7."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    s = f32(D ** -0.5 if scale is None else scale)
    bounds = [0, T] if cu is None else [int(b) for b in cu.tolist()]
    pairs = [(int(r), int(c)) for r, c in pairs]
    assert len({r for r, _ in pairs}) == len(pairs) == len({c for _, c in pairs})

    def span(r, c):
        if past:
            assert c <= past + r, (r, c)
            return 0, (past + r + 1 if causal else k.shape[0]), c
        a, b = next((a, b) for a, b in zip(bounds[:-1], bounds[1:]) if a <= r < b)
        assert a <= c < b and (not causal or c <= r), (r, c)
        return a, (r + 1 if causal else b), c

    def scores(r, c, h):
        lo, hi, _ = span(r, c)
        return torch.mv(k[lo:hi, h].double(), q[r, probe_targets(Hkv, G)[h]].double()) * s, c - lo

    got = torch.zeros((len(pairs), Hkv), dtype=torch.float64)
    for step in range(3):
        for i, (r, c) in enumerate(pairs):
            for h, tgt in enumerate(probe_targets(Hkv, G)):
                x, j = scores(r, c, h)
                if step == 2:
                    got[i, h] = float(torch.softmax(x, 0)[j])
                    continue
                rest = torch.cat((x[:j], x[j + 1:]))
                assert rest.numel() > 0, f"row {r} sees no key but its own: its weight is 1 whatever alpha"
                want = float(torch.logsumexp(rest, 0)) + float(torch.log(torch.tensor(weight / (1.0 - weight), dtype=torch.float64)))
                n2 = float(q[r, tgt].double().pow(2).sum()) * s
                k[c, h] = (want / n2 * q[r, tgt].float()).to(torch.bfloat16)
    return got


def framed_thd(T: int, H: int, D: int, ld_pad: int = 8, guard_rows: int = 3, dtype=torch.bfloat16, device="cuda"):
    """-> (view [T, H, D], check): framed_out's [T, H * D] view with the heads split off (strides ld, D, 1)."""
    view, check = framed_out(T, H * D, ld_pad, guard_rows, dtype=dtype, device=device)
    return view.unflatten(1, (H, D)), check


def framed_thd_operand(t: torch.Tensor, ld_pad: int = 8, guard_rows: int = 3) -> torch.Tensor:
    """t [T, H, D] -> the same values as a [T, H, D] view of framed_operand's NaN-padded buffer."""
    T, H, D = t.shape
    return framed_operand(t.reshape(T, H * D), ld_pad, guard_rows).unflatten(1, (H, D))

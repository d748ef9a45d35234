"""Operator-level Python wrappers over the C-ABI (device pointers + the current HIP stream).  PyTorch only owns
the buffers.  Every op raises on CPU tensors: there is no fallback path."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check

EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF, EPI_GATEUP = 0, 1, 2, 3


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(t: torch.Tensor, dtype=torch.bfloat16, name: str = "tensor") -> None:
    if not t.is_cuda:
        raise _lib.VilaHipError(f"{name} must live on the GPU: vila_amd has no CPU path (got device {t.device})")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         epi: int = EPI_NONE, w2: Optional[torch.Tensor] = None, out_f32: bool = False,
         out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias) + residual   (nn.Linear semantics; EPI_GATEUP: silu(a w^T) * (a w2^T))."""
    _need(a, name="a"); _need(w, name="w")
    # w may carry extra zero-padded columns (transpose() pads the contraction dim to 64): K is a's width
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1
    if a.shape[1] != w.shape[1] and w.shape[1] != (a.shape[1] + 63) // 64 * 64:
        raise ValueError(f"gemm: contraction widths differ (a: {a.shape[1]}, w: {w.shape[1]}); only the zero padding of transpose() to a "
                         "multiple of 64 is accepted")
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    if residual is not None:
        _need(residual, name="residual"); assert residual.shape == (M, N) and residual.stride(1) == 1
    if ws is not None:   # fp32 workspace: allows split-K on under-filled grids
        check(_lib.load().vila_gemm_bf16_ws(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(w2), _p(bias), _p(residual),
                                            residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0),
                                            1 if out_f32 else 0, M, N, K, epi, ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
              "vila_gemm_bf16_ws")
        return out
    check(_lib.load().vila_gemm_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(w2), _p(bias), _p(residual),
                                     residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0),
                                     1 if out_f32 else 0, M, N, K, epi, _stream()), "vila_gemm_bf16")
    return out


def gemm_t(a: torch.Tensor, w: torch.Tensor, a_cm: bool = False, b_cm: bool = False, bias: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = A . B^T (+bias)(+residual) with operands read as they lie: a_cm -> `a` is stored [K, M], b_cm -> `w` is stored [K, N]
    (vila_gemm_bf16_t).  dgrad: gemm_t(dy, W, b_cm=True);  wgrad: gemm_t(dy, x, a_cm=True, b_cm=True)."""
    _need(a, name="a"); _need(w, name="w")
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1
    M, K = (a.shape[1], a.shape[0]) if a_cm else a.shape
    N, Kw = (w.shape[1], w.shape[0]) if b_cm else w.shape
    if K != Kw:
        raise ValueError(f"gemm_t: contraction widths differ ({K} vs {Kw})")
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.bfloat16)
    assert out.shape == (M, N) and out.stride(1) == 1
    if residual is not None:
        _need(residual, name="residual"); assert residual.shape == (M, N) and residual.stride(1) == 1
    check(_lib.load().vila_gemm_bf16_t(a.data_ptr(), a.stride(0), int(a_cm), w.data_ptr(), w.stride(0), int(b_cm), _p(bias), _p(residual),
                                       residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), M, N, K,
                                       _p(ws), ws.numel() * ws.element_size() if ws is not None else 0, _stream()), "vila_gemm_bf16_t")
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    _need(x, name="x")
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    y = torch.empty_like(x2)
    check(_lib.load().vila_layernorm_bf16(x2.data_ptr(), w.data_ptr(), _p(b), y.data_ptr(), x2.shape[0], x2.shape[1], eps, _stream()), "layernorm")
    return y.view(x.shape)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    _need(x, name="x")
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    y = torch.empty_like(x2)
    check(_lib.load().vila_rmsnorm_bf16(x2.data_ptr(), w.data_ptr(), y.data_ptr(), x2.shape[0], x2.shape[1], eps, _stream()), "rmsnorm")
    return y.view(x.shape)


def space_to_depth(x: torch.Tensor, k: int) -> torch.Tensor:
    """[B, g*g, C] -> [B, ceil(g/k)^2, k*k*C]  (flat_square / flat_square_2x2 / flat_square_3x3)."""
    _need(x, name="x")
    B, N, Cc = x.shape
    g = int(round(N ** 0.5))
    assert g * g == N
    gd = (g + k - 1) // k
    y = torch.empty((B, gd * gd, k * k * Cc), device=x.device, dtype=x.dtype)
    check(_lib.load().vila_space_to_depth_bf16(x.contiguous().data_ptr(), y.data_ptr(), B, g, Cc, k, _stream()), "space_to_depth")
    return y


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool, scale: Optional[float] = None,
             cu_seqlens: Optional[torch.Tensor] = None, max_seqlen: Optional[int] = None, n_seq: int = 1,
             return_lse: bool = False):
    """q [T, Hq, D], k/v [T, Hkv, D] (last dim contiguous; token/head strides free) -> o [T, Hq, D] (+ lse [Hq, T])."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _need(t, name=n); assert t.dim() == 3 and t.stride(2) == 1
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    if scale is None:
        scale = D ** -0.5
    if cu_seqlens is not None:
        assert cu_seqlens.dtype == torch.int32 and cu_seqlens.is_cuda
        n_seq = cu_seqlens.numel() - 1
        assert max_seqlen is not None
    else:
        max_seqlen = T // n_seq
    o = torch.empty((T, Hq, D), device=q.device, dtype=q.dtype)
    lse = torch.empty((Hq, T), device=q.device, dtype=torch.float32) if return_lse else None
    check(_lib.load().vila_attn_fwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(0), k.stride(0),
                                         v.stride(0), o.stride(0), q.stride(1), k.stride(1), v.stride(1), o.stride(1),
                                         _p(cu_seqlens), n_seq, T, max_seqlen, Hq, Hkv, D, 1 if causal else 0, float(scale),
                                         _p(lse), _stream()), "attn_fwd")
    return (o, lse) if return_lse else o


def gemv(x: torch.Tensor, w: torch.Tensor, norm_w: Optional[torch.Tensor] = None, eps: float = 0.0,
         w2: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         out_f32: bool = False) -> torch.Tensor:
    _need(x, name="x"); _need(w, name="w")
    N, K = w.shape
    y = torch.empty((N,), device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    check(_lib.load().vila_gemv_bf16(x.data_ptr(), _p(norm_w), eps, w.data_ptr(), _p(w2), _p(bias), _p(residual),
                                     None if out_f32 else y.data_ptr(), y.data_ptr() if out_f32 else None, N, K,
                                     1 if w2 is not None else 0, _stream()), "gemv")
    return y


def gemv_w4(x: torch.Tensor, mat, norm_w: Optional[torch.Tensor] = None, eps: float = 0.0, bias: Optional[torch.Tensor] = None,
            residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W4A16 GEMV on a vila_amd.quant.W4Matrix (tile-major int4, group 128); gate/up matrices give silu(Wg x) * (Wu x).  `out` [N] bf16
    contiguous: written in place of a fresh result."""
    _need(x, name="x"); _need(mat.q, dtype=torch.int32, name="mat.q"); _need(mat.sz, dtype=torch.int32, name="mat.sz")
    if x.numel() != mat.K:
        raise ValueError(f"gemv_w4: x has {x.numel()} elements, the matrix K = {mat.K}")
    y = torch.empty((mat.N,), device=x.device, dtype=torch.bfloat16) if out is None else out
    _need(y, name="out"); assert y.shape == (mat.N,) and y.is_contiguous()
    check(_lib.load().vila_gemv_w4_bf16(x.data_ptr(), _p(norm_w), eps, mat.q.data_ptr(), mat.sz.data_ptr(), _p(bias), _p(residual),
                                        y.data_ptr(), mat.N, mat.K, mat.mode, _stream()), "gemv_w4")
    return y


def qkv_w4(x: torch.Tensor, mat, bias: Optional[torch.Tensor], q_out: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, pos: torch.Tensor,
           rope_cs: torch.Tensor, q_heads: int, kv_heads: int, head_dim: int, norm_w: Optional[torch.Tensor] = None, eps: float = 0.0) -> torch.Tensor:
    """The solo W4A16 decode step's fused q|k|v projection (vila_qkv_w4_bf16, gemv_w4.hip mode 3): x [K] bf16 (optionally RMS-normalised with norm_w,
    eps), mat a plain W4Matrix of the (q + 2 kv) * head_dim fused rows packed with quant.rope_interleave_rows; bias [N] in natural order; RoPE from
    rope_cs [head_dim] fp32 (cos | sin); q into q_out [q * head_dim], K / V into row pos[0] (device int32) of kcache / vcache [kv, max_ctx, head_dim];
    pos[0] >= max_ctx writes q and no K/V."""
    _need(x, name="x"); _need(mat.q, dtype=torch.int32, name="mat.q"); _need(mat.sz, dtype=torch.int32, name="mat.sz")
    _need(q_out, name="q_out"); _need(kcache, name="kcache"); _need(vcache, name="vcache")
    _need(pos, dtype=torch.int32, name="pos"); _need(rope_cs, dtype=torch.float32, name="rope_cs")
    if x.numel() != mat.K:
        raise ValueError(f"qkv_w4: x has {x.numel()} elements, the matrix K = {mat.K}")
    if mat.mode != 0 or mat.N != (q_heads + 2 * kv_heads) * head_dim:
        raise ValueError(f"qkv_w4: heads ({q_heads}, {kv_heads}, {head_dim}) describe {(q_heads + 2 * kv_heads) * head_dim} q|k|v rows, the matrix has "
                         f"{mat.N} (mode {mat.mode})")
    assert x.is_contiguous() and q_out.is_contiguous() and q_out.numel() >= q_heads * head_dim
    assert kcache.dim() == 3 and kcache.shape == vcache.shape and kcache.shape[0] == kv_heads and kcache.shape[2] == head_dim
    assert kcache.is_contiguous() and vcache.is_contiguous() and pos.numel() >= 1 and rope_cs.is_contiguous() and rope_cs.numel() >= head_dim
    check(_lib.load().vila_qkv_w4_bf16(x.data_ptr(), _p(norm_w), eps, mat.q.data_ptr(), mat.sz.data_ptr(), _p(bias), q_out.data_ptr(), kcache.data_ptr(),
                                       vcache.data_ptr(), pos.data_ptr(), rope_cs.data_ptr(), q_heads, kv_heads, head_dim, kcache.shape[1], mat.K,
                                       _stream()), "qkv_w4")
    return q_out


def gemv_w4_batch(x: torch.Tensor, mat, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, n: Optional[int] = None) -> torch.Tensor:
    """W4A16 batched decode GEMV on a vila_amd.quant.W4Matrix: x [n, K] bf16 (1 <= n <= 16 rows, any row stride that is a multiple of 8) ->
    [n, N] bf16 = x . W^T (+bias)(+residual [>= n, N]); gate/up matrices give silu(x Wg^T) * (x Wu^T) and take no bias or residual.  `out` and
    `residual` have row stride N (the entry point fixes it) and may be views of larger buffers (guard rows around them, more rows than n; the
    residual may be `out`).  Rows of `out` beyond n are not written.  `n` overrides x's row count (the refusals are reachable with it)."""
    _need(x, name="x"); _need(mat.q, dtype=torch.int32, name="mat.q"); _need(mat.sz, dtype=torch.int32, name="mat.sz")
    assert x.dim() == 2 and x.stride(1) == 1
    if x.shape[1] != mat.K:
        raise ValueError(f"gemv_w4_batch: x has {x.shape[1]} columns, the matrix {mat.K}")
    n = x.shape[0] if n is None else n
    if out is None:
        out = torch.empty((n, mat.N), device=x.device, dtype=torch.bfloat16)
    for t, name in ((out, "out"), (residual, "residual")):
        if t is not None:
            _need(t, name=name); assert t.dim() == 2 and t.is_contiguous() and t.shape[1] == mat.N and t.shape[0] >= min(n, 16)
    check(_lib.load().vila_gemv_w4_batch_bf16(x.data_ptr(), x.stride(0), n, mat.q.data_ptr(), mat.sz.data_ptr(), _p(bias), _p(residual),
                                              out.data_ptr(), mat.N, mat.K, mat.mode, _stream()), "gemv_w4_batch")
    return out


def qkv_w4_batch(x: torch.Tensor, mat, bias: Optional[torch.Tensor], q_out: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                 pos: torch.Tensor, rope_cs: torch.Tensor, q_heads: int, kv_heads: int, head_dim: int, n: Optional[int] = None) -> torch.Tensor:
    """The batched W4A16 decode step's q|k|v projection (vila_qkv_w4_batch_bf16, gemv_w4_batch.hip mode 2): qkv_batch's arguments with a plain
    W4Matrix of the fused rows, packed with quant.rope_interleave_rows, in place of wqkv; same contract."""
    _need(x, name="x"); _need(mat.q, dtype=torch.int32, name="mat.q"); _need(mat.sz, dtype=torch.int32, name="mat.sz")
    _need(q_out, name="q_out"); _need(kcache, name="kcache"); _need(vcache, name="vcache")
    _need(pos, dtype=torch.int32, name="pos"); _need(rope_cs, dtype=torch.float32, name="rope_cs")
    assert x.dim() == 2 and x.stride(1) == 1 and q_out.dim() == 2 and q_out.stride(1) == 1
    if x.shape[1] != mat.K:
        raise ValueError(f"qkv_w4_batch: x has {x.shape[1]} columns, the matrix {mat.K}")
    if mat.mode != 0 or mat.N != (q_heads + 2 * kv_heads) * head_dim:
        raise ValueError(f"qkv_w4_batch: heads ({q_heads}, {kv_heads}, {head_dim}) describe {(q_heads + 2 * kv_heads) * head_dim} q|k|v rows, the matrix "
                         f"has {mat.N} (mode {mat.mode})")
    n = x.shape[0] if n is None else n
    assert q_out.shape[1] == q_heads * head_dim and q_out.shape[0] >= min(n, 16)
    assert kcache.dim() == 4 and kcache.shape == vcache.shape and kcache.shape[1:] == (kv_heads, kcache.shape[2], head_dim) and kcache.shape[0] >= min(n, 16)
    assert kcache[0].is_contiguous() and vcache[0].is_contiguous() and kcache.stride(0) == vcache.stride(0)
    assert pos.numel() >= min(n, 16) and rope_cs.is_contiguous() and rope_cs.numel() >= min(n, 16) * head_dim
    check(_lib.load().vila_qkv_w4_batch_bf16(x.data_ptr(), x.stride(0), n, mat.q.data_ptr(), mat.sz.data_ptr(), _p(bias), q_out.data_ptr(),
                                             q_out.stride(0), kcache.data_ptr(), vcache.data_ptr(), kcache.stride(0), pos.data_ptr(), rope_cs.data_ptr(),
                                             q_heads, kv_heads, head_dim, kcache.shape[2], mat.K, _stream()), "qkv_w4_batch")
    return q_out


def gemm_batch(x: torch.Tensor, w: torch.Tensor, w2: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None,
               n: Optional[int] = None) -> Optional[torch.Tensor]:
    """The batched decode step's skinny GEMM (vila_gemm_batch_bf16): x [n, K] bf16 (1 <= n <= 16, any row stride that is a multiple of 8),
    w [N, K] contiguous -> out [>= n, N] bf16 = x . w^T (+bias)(+residual; may be `out`) and/or out_f32 [>= n, N] fp32 (the sum before any rounding);
    with w2: out = silu(x w^T) * (x w2^T).  Without `out` and `out_f32` a bf16 result is allocated.  Rows of the outputs beyond n are not written.
    `n` overrides x's row count (the refusals of the entry point are reachable with it)."""
    _need(x, name="x"); _need(w, name="w")
    assert x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1 and w.is_contiguous() and (w2 is None or (w2.is_contiguous() and w2.shape == w.shape))
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"gemm_batch: x has {x.shape[1]} columns, the matrix {w.shape[1]}")
    n = x.shape[0] if n is None else n
    N, K = w.shape
    if out is None and out_f32 is None:
        out = torch.empty((n, N), device=x.device, dtype=torch.bfloat16)
    for t, dt, name in ((out, torch.bfloat16, "out"), (out_f32, torch.float32, "out_f32"), (residual, torch.bfloat16, "residual")):
        if t is not None:
            _need(t, dtype=dt, name=name); assert t.dim() == 2 and t.stride(1) == 1 and t.shape[1] == N and t.shape[0] >= min(n, 16)
    ld = lambda t: 0 if t is None else t.stride(0)
    check(_lib.load().vila_gemm_batch_bf16(x.data_ptr(), x.stride(0), n, w.data_ptr(), _p(w2), _p(bias), _p(residual), ld(residual), _p(out), ld(out),
                                           _p(out_f32), ld(out_f32), N, K, _stream()), "gemm_batch")
    return out if out is not None else out_f32


def qkv_batch(x: torch.Tensor, wqkv: torch.Tensor, bias: Optional[torch.Tensor], q_out: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
              pos: torch.Tensor, rope_cs: torch.Tensor, q_heads: int, kv_heads: int, head_dim: int, n: Optional[int] = None) -> torch.Tensor:
    """The batched decode step's q|k|v projection (vila_qkv_batch_bf16): x [n, K] bf16, wqkv [(q + 2 kv) * head_dim, K] contiguous; row m gets the
    bias, RoPE from rope_cs [n, head_dim] fp32 (cos | sin of its position), q into q_out [>= n, q * head_dim] and K / V into row pos[m] (int32) of
    kcache / vcache [slots >= n, kv, max_ctx, head_dim] slot m; rows with pos[m] >= max_ctx write no K/V."""
    _need(x, name="x"); _need(wqkv, name="wqkv"); _need(q_out, name="q_out"); _need(kcache, name="kcache"); _need(vcache, name="vcache")
    _need(pos, dtype=torch.int32, name="pos"); _need(rope_cs, dtype=torch.float32, name="rope_cs")
    assert x.dim() == 2 and x.stride(1) == 1 and wqkv.is_contiguous() and q_out.dim() == 2 and q_out.stride(1) == 1
    if x.shape[1] != wqkv.shape[1]:
        raise ValueError(f"qkv_batch: x has {x.shape[1]} columns, the matrix {wqkv.shape[1]}")
    n = x.shape[0] if n is None else n
    assert wqkv.shape[0] == (q_heads + 2 * kv_heads) * head_dim and q_out.shape[1] == q_heads * head_dim and q_out.shape[0] >= min(n, 16)
    assert kcache.dim() == 4 and kcache.shape == vcache.shape and kcache.shape[1:] == (kv_heads, kcache.shape[2], head_dim) and kcache.shape[0] >= min(n, 16)
    assert kcache[0].is_contiguous() and vcache[0].is_contiguous() and kcache.stride(0) == vcache.stride(0)
    assert pos.numel() >= min(n, 16) and rope_cs.is_contiguous() and rope_cs.numel() >= min(n, 16) * head_dim
    check(_lib.load().vila_qkv_batch_bf16(x.data_ptr(), x.stride(0), n, wqkv.data_ptr(), _p(bias), q_out.data_ptr(), q_out.stride(0), kcache.data_ptr(),
                                          vcache.data_ptr(), kcache.stride(0), pos.data_ptr(), rope_cs.data_ptr(), q_heads, kv_heads, head_dim,
                                          kcache.shape[2], x.shape[1], _stream()), "qkv_batch")
    return q_out


def _addend_args(addend, row_adapter, n: int, width: int, what: str):
    """(addend pointer, row stride, row_adapter pointer) of an entry that takes the adapters' fp32 addend [>= n, width] and the rows' slots [>= n] int32."""
    if addend is None:
        return None, 0, _p(row_adapter)
    _need(addend, dtype=torch.float32, name="addend")
    assert addend.dim() == 2 and addend.stride(1) == 1 and addend.shape[1] == width and addend.shape[0] >= min(n, 16), what
    if row_adapter is not None:
        _need(row_adapter, dtype=torch.int32, name="row_adapter"); assert row_adapter.numel() >= min(n, 16)
    return addend.data_ptr(), addend.stride(0), _p(row_adapter)


def gemm_batch_lora(x: torch.Tensor, w: torch.Tensor, addend: Optional[torch.Tensor], row_adapter: Optional[torch.Tensor],
                    w2: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None, n: Optional[int] = None) -> Optional[torch.Tensor]:
    """gemm_batch with the fp32 addend of a step with per-row adapters (vila_gemm_batch_lora_bf16; with w2 vila_gateup_batch_lora_bf16): addend
    [>= n, N] (gate/up: [>= n, 2 N], gate | up) joins the fp32 sum in front of the bias and the first rounding; a row with row_adapter[m] < 0 skips
    the add.  addend None launches gemm_batch's kernels."""
    _need(x, name="x"); _need(w, name="w")
    assert x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1 and w.is_contiguous() and (w2 is None or (w2.is_contiguous() and w2.shape == w.shape))
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"gemm_batch_lora: x has {x.shape[1]} columns, the matrix {w.shape[1]}")
    n = x.shape[0] if n is None else n
    N, K = w.shape
    if out is None and out_f32 is None:
        out = torch.empty((n, N), device=x.device, dtype=torch.bfloat16)
    for t, dt, name in ((out, torch.bfloat16, "out"), (out_f32, torch.float32, "out_f32"), (residual, torch.bfloat16, "residual")):
        if t is not None:
            _need(t, dtype=dt, name=name); assert t.dim() == 2 and t.stride(1) == 1 and t.shape[1] == N and t.shape[0] >= min(n, 16)
    ld = lambda t: 0 if t is None else t.stride(0)
    ap, lda, rp = _addend_args(addend, row_adapter, n, 2 * N if w2 is not None else N, "gemm_batch_lora")
    if w2 is not None:
        assert bias is None and residual is None and out_f32 is None, "gate/up takes no bias, residual or fp32 output"
        check(_lib.load().vila_gateup_batch_lora_bf16(x.data_ptr(), x.stride(0), n, w.data_ptr(), w2.data_ptr(), out.data_ptr(), ld(out), N, K, ap, lda, rp,
                                                      _stream()), "gemm_batch_lora")
    else:
        check(_lib.load().vila_gemm_batch_lora_bf16(x.data_ptr(), x.stride(0), n, w.data_ptr(), _p(bias), _p(residual), ld(residual), _p(out), ld(out),
                                                    _p(out_f32), ld(out_f32), N, K, ap, lda, rp, _stream()), "gemm_batch_lora")
    return out if out is not None else out_f32


def qkv_batch_lora(x: torch.Tensor, wqkv: torch.Tensor, bias: Optional[torch.Tensor], q_out: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                   pos: torch.Tensor, rope_cs: torch.Tensor, q_heads: int, kv_heads: int, head_dim: int, addend: Optional[torch.Tensor],
                   row_adapter: Optional[torch.Tensor], n: Optional[int] = None) -> torch.Tensor:
    """qkv_batch with the adapters' fp32 addend [>= n, (q + 2 kv) * head_dim] in front of the bias, RoPE and the cache append (vila_qkv_batch_lora_bf16)."""
    _need(x, name="x"); _need(wqkv, name="wqkv"); _need(q_out, name="q_out"); _need(kcache, name="kcache"); _need(vcache, name="vcache")
    _need(pos, dtype=torch.int32, name="pos"); _need(rope_cs, dtype=torch.float32, name="rope_cs")
    assert x.dim() == 2 and x.stride(1) == 1 and wqkv.is_contiguous() and q_out.dim() == 2 and q_out.stride(1) == 1
    if x.shape[1] != wqkv.shape[1]:
        raise ValueError(f"qkv_batch_lora: x has {x.shape[1]} columns, the matrix {wqkv.shape[1]}")
    n = x.shape[0] if n is None else n
    assert wqkv.shape[0] == (q_heads + 2 * kv_heads) * head_dim and q_out.shape[1] == q_heads * head_dim and q_out.shape[0] >= min(n, 16)
    assert kcache.dim() == 4 and kcache.shape == vcache.shape and kcache.shape[1:] == (kv_heads, kcache.shape[2], head_dim) and kcache.shape[0] >= min(n, 16)
    assert kcache[0].is_contiguous() and vcache[0].is_contiguous() and kcache.stride(0) == vcache.stride(0)
    assert pos.numel() >= min(n, 16) and rope_cs.is_contiguous() and rope_cs.numel() >= min(n, 16) * head_dim
    ap, lda, rp = _addend_args(addend, row_adapter, n, wqkv.shape[0], "qkv_batch_lora")
    check(_lib.load().vila_qkv_batch_lora_bf16(x.data_ptr(), x.stride(0), n, wqkv.data_ptr(), _p(bias), q_out.data_ptr(), q_out.stride(0), kcache.data_ptr(),
                                               vcache.data_ptr(), kcache.stride(0), pos.data_ptr(), rope_cs.data_ptr(), q_heads, kv_heads, head_dim,
                                               kcache.shape[2], x.shape[1], ap, lda, rp, _stream()), "qkv_batch_lora")
    return q_out


def lora_shrink(x: torch.Tensor, a_bank: torch.Tensor, scale: torch.Tensor, row_adapter: torch.Tensor, out: torch.Tensor,
                n: Optional[int] = None) -> torch.Tensor:
    """The shrink of the step with per-row adapters (vila_lora_shrink_bf16): x [n, K] bf16, a_bank [capacity, Rs, K] bf16 (slots may be strided),
    scale [capacity] fp32, row_adapter [n] int32 -> out [>= n, Rs] fp32 = scale[a] * x_i . A_a^T with a = row_adapter[i]; +0.0 for a row without."""
    _need(x, name="x"); _need(a_bank, name="a_bank"); _need(scale, dtype=torch.float32, name="scale"); _need(row_adapter, dtype=torch.int32, name="row_adapter")
    _need(out, dtype=torch.float32, name="out")
    assert x.dim() == 2 and x.stride(1) == 1 and a_bank.dim() == 3 and a_bank[0].is_contiguous() and out.dim() == 2 and out.stride(1) == 1
    cap, Rs, K = a_bank.shape
    if x.shape[1] != K:
        raise ValueError(f"lora_shrink: x has {x.shape[1]} columns, the bank's A {K}")
    n = x.shape[0] if n is None else n
    assert out.shape[1] == Rs and out.shape[0] >= min(n, 16) and scale.numel() >= cap and row_adapter.numel() >= min(n, 16)
    check(_lib.load().vila_lora_shrink_bf16(x.data_ptr(), x.stride(0), n, a_bank.data_ptr(), a_bank.stride(0), scale.data_ptr(), row_adapter.data_ptr(), cap,
                                            out.data_ptr(), out.stride(0), Rs, K, _stream()), "lora_shrink")
    return out


def lora_expand(t: torch.Tensor, b_bank: torch.Tensor, row_adapter: torch.Tensor, out: torch.Tensor, c1: Optional[int] = None, c2: Optional[int] = None,
                n: Optional[int] = None) -> torch.Tensor:
    """The expand of the step with per-row adapters (vila_lora_expand_f32): t [n, segments * r] fp32, b_bank [capacity, r / 8, N, 8] bf16 (lora_B of
    the stack's members side by side, chunk-major), row_adapter [n] int32 -> out [>= n, N] fp32.  Columns [0, c1) read t[:, 0:r], [c1, c2) t[:, r:2r],
    [c2, N) t[:, 2r:3r]; c1 = c2 = N (the default): one member."""
    _need(t, dtype=torch.float32, name="t"); _need(b_bank, name="b_bank"); _need(row_adapter, dtype=torch.int32, name="row_adapter")
    _need(out, dtype=torch.float32, name="out")
    assert t.dim() == 2 and t.stride(1) == 1 and b_bank.dim() == 4 and b_bank.shape[3] == 8 and b_bank[0].is_contiguous() and out.dim() == 2 and out.stride(1) == 1
    cap, chunks, N, _ = b_bank.shape
    c1 = N if c1 is None else int(c1)
    c2 = N if c2 is None else int(c2)
    n = t.shape[0] if n is None else n
    assert out.shape[1] == N and out.shape[0] >= min(n, 16) and row_adapter.numel() >= min(n, 16)
    assert t.shape[1] == (1 + (c1 < N) + (c2 < N)) * chunks * 8, "t holds one r-wide slice per member of the stack"
    check(_lib.load().vila_lora_expand_f32(t.data_ptr(), t.stride(0), n, b_bank.data_ptr(), b_bank.stride(0), row_adapter.data_ptr(), cap, out.data_ptr(),
                                           out.stride(0), N, chunks * 8, c1, c2, _stream()), "lora_expand")
    return out


def gemm_w4(x: torch.Tensor, mat, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, heads: Optional[tuple] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W4A16 GEMM (prefill shapes) on a vila_amd.quant.W4Matrix: x [M, K] bf16 -> [M, N] bf16 = x . W^T (+bias)(+residual); gate/up
    matrices give silu(x Wg^T) * (x Wu^T).  heads = (q_heads, kv_heads, head_dim) marks the fused q|k|v matrix of a W4 layer (rows of the
    q and k heads RoPE-interleaved): the result comes back in natural q | k | v column order with the bias added.  `ws`: a caller's uint8 workspace
    of at least vila_gemm_w4_workspace_bytes (one is allocated otherwise)."""
    _need(x, name="x"); _need(mat.q, dtype=torch.int32, name="mat.q"); _need(mat.sz, dtype=torch.int32, name="mat.sz")
    assert x.dim() == 2 and x.is_contiguous()
    if x.shape[1] != mat.K:
        raise ValueError(f"gemm_w4: x has {x.shape[1]} columns, the matrix {mat.K}")
    M = x.shape[0]
    lib = _lib.load()
    mode = 2 if heads is not None else mat.mode
    if out is None:
        out = torch.empty((M, mat.N), device=x.device, dtype=torch.bfloat16)
    if residual is not None:
        _need(residual, name="residual"); assert residual.shape == (M, mat.N) and residual.is_contiguous()
    nb = lib.vila_gemm_w4_workspace_bytes(M, mat.N, mat.K, mode)
    if ws is None:
        ws = torch.empty((max(nb, 1),), device=x.device, dtype=torch.uint8)
    else:
        _need(ws, dtype=torch.uint8, name="ws"); assert ws.is_contiguous()
        nb = ws.numel()
    if heads is not None:
        nq, nkv, hd = (int(v) for v in heads)
        if (nq + 2 * nkv) * hd != mat.N or mat.mode != 0:
            raise ValueError(f"gemm_w4: heads {tuple(heads)} describe {(nq + 2 * nkv) * hd} q|k|v rows, the matrix has {mat.N} (mode {mat.mode})")
        if residual is not None:
            raise ValueError("gemm_w4: the q|k|v form takes no residual")
        check(lib.vila_gemm_w4_qkv_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), _p(bias), out.data_ptr(), M, nq, nkv, hd, mat.K,
                                        ws.data_ptr(), nb, _stream()), "gemm_w4_qkv")
        return out
    check(lib.vila_gemm_w4_bf16(x.data_ptr(), mat.q.data_ptr(), mat.sz.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, mat.N, mat.K,
                                mat.mode, ws.data_ptr(), nb, _stream()), "gemm_w4")
    return out


def argmax(logits: torch.Tensor) -> torch.Tensor:
    _need(logits, dtype=torch.float32, name="logits")
    out = torch.empty((1,), device=logits.device, dtype=torch.int64)
    ws = torch.empty((4096,), device=logits.device, dtype=torch.uint8)
    check(_lib.load().vila_argmax_f32(logits.data_ptr(), logits.numel(), out.data_ptr(), ws.data_ptr(), _stream()), "argmax")
    return out


def wave_sum_probe(x: torch.Tensor):
    """Both wave reductions of the decode GEMVs over every 64 consecutive fp32 inputs: (LDS-free xor butterfly, shuffle butterfly), each
    the size of x, every lane's own result."""
    _need(x, dtype=torch.float32, name="x")
    if x.numel() == 0 or x.numel() % 64:
        raise ValueError(f"wave_sum_probe: {x.numel()} inputs are not whole waves of 64")
    a, b = torch.empty_like(x), torch.empty_like(x)
    check(_lib.load().vila_wave_sum_probe(x.data_ptr(), a.data_ptr(), b.data_ptr(), x.numel() // 64, _stream()), "wave_sum_probe")
    return a, b


def sample(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, seed: int = 0,
           counter: Optional[torch.Tensor] = None, return_dist: bool = False):
    """HF sampling on the device (GenerationMixin.sample): logits / temperature -> TopK (any k >= 1; 0 = no top-k filter, as HF treats it) ->
    TopP -> softmax -> draw with splitmix64(seed, *counter).  -> token id [1] i64 (and, on request, the distribution that was sampled as
    (probabilities, token ids): 64 slots for top_k in 1..64, the dense vocabulary otherwise)."""
    _need(logits, dtype=torch.float32, name="logits")
    lib = _lib.load()
    out = torch.empty((1,), device=logits.device, dtype=torch.int64)
    ws = torch.empty((lib.vila_sample_workspace_bytes(),), device=logits.device, dtype=torch.uint8)
    small = 1 <= int(top_k) <= 64
    dist = torch.zeros((128 if small else logits.numel(),), device=logits.device, dtype=torch.float32) if return_dist else None
    sp = _lib.VilaSampling(float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF)
    import ctypes as C
    check(lib.vila_sample_f32(logits.data_ptr(), logits.numel(), C.byref(sp), _p(counter), out.data_ptr(), ws.data_ptr(), _p(dist), _stream()), "sample")
    if return_dist:
        if small:
            return out, dist[:64].clone(), dist[64:].view(torch.int32).clone()
        return out, dist, torch.arange(logits.numel(), device=logits.device, dtype=torch.int32)
    return out


def sample_batch(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
                 counter: Optional[torch.Tensor] = None, return_dist: bool = False, any_top_k: bool = False, return_dense: bool = False):
    """`sample` for up to 16 rows at once (the pick of the batched decode step): logits [n, V] fp32 (rows may be strided), every parameter a
    DEVICE tensor [n] — temperature f32 (<= 0: greedy row = argmax, ties to the lower index), top_k i32 in 1..64, top_p f32 in (0, 1], seed i64
    (the bit pattern of a uint64), counter i32 (optional).  A sampled row gets bit for bit the token `sample` returns for that row.
    any_top_k (opt-in; default False = the call and the clamp of top_k to 1..64 as ever): `vila_sample_batch_any_f32` — a row with top_k = 0 (no
    top-k filter) or top_k > 64 is drawn by `sample`'s exact path for such a k, one launch more; its entries of the 64-slot distribution are zeros
    and -1 ids.  return_dense (with any_top_k): also the dense distributions [n, V] fp32, of which only such rows are written (the others stay 0).
    -> token ids [n] i64 (and, on request, (probabilities [n, 64], token ids [n, 64] i32), then the dense distributions)."""
    _need(logits, dtype=torch.float32, name="logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("sample_batch: logits must be [n, vocab] with contiguous rows")
    if return_dense and not any_top_k:
        raise ValueError("sample_batch: return_dense is the dense distribution of the rows any_top_k=True draws")
    n, V = logits.shape
    for name, t, dt in (("temperature", temperature, torch.float32), ("top_k", top_k, torch.int32), ("top_p", top_p, torch.float32),
                        ("seed", seed, torch.int64)) + ((("counter", counter, torch.int32),) if counter is not None else ()):
        _need(t, dtype=dt, name=name)
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"sample_batch: {name} must be a contiguous tensor of {n} entries")
    import ctypes as C
    lib = _lib.load()
    out = torch.empty((n,), device=logits.device, dtype=torch.int64)
    ws = torch.empty((lib.vila_sample_batch_workspace_bytes(n),), device=logits.device, dtype=torch.uint8)
    dist = torch.zeros((n, 128), device=logits.device, dtype=torch.float32) if return_dist else None
    sp = _lib.VilaBatchSampling(temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), seed.data_ptr())
    dense = None
    if any_top_k:
        dense = torch.zeros((n, V), device=logits.device, dtype=torch.float32) if return_dense else None
        check(lib.vila_sample_batch_any_f32(logits.data_ptr(), logits.stride(0), n, V, C.byref(sp), _p(counter), out.data_ptr(), ws.data_ptr(), _p(dist),
                                            _p(dense), V, _stream()), "sample_batch_any")
    else:
        check(lib.vila_sample_batch_f32(logits.data_ptr(), logits.stride(0), n, V, C.byref(sp), _p(counter), out.data_ptr(), ws.data_ptr(), _p(dist),
                                        _stream()), "sample_batch")
    res = (out,)
    if return_dist:
        res += (dist[:, :64].clone(), dist[:, 64:].contiguous().view(torch.int32))
    if return_dense:
        res += (dense,)
    return res if len(res) > 1 else out


def penalize(logits: torch.Tensor, counts: torch.Tensor, repetition: torch.Tensor, presence: torch.Tensor, frequency: torch.Tensor,
             token: Optional[torch.Tensor] = None, return_pick: bool = False):
    """Repetition / presence / frequency penalties on logits [n, V] fp32 (rows may be strided): the launch the penalised decode steps run between the
    logits and the pick.  counts [n, >= V] int16 or uint16 (the bits of uint16 counters; rows may be strided) = how often each row's request has
    generated each id; token [n] i64 (optional): counts[r, token[r]] is bumped first (saturating at 65535; an id outside 0 .. V - 1 bumps nothing).
    repetition / presence / frequency: DEVICE tensors [n] f32.  Where c = counts[r, i] > 0: y = x * rep if x < 0 else x / rep; then
    y -= frequency * c; then y -= presence where c > 0 — each one rounded fp32 operation, bit for bit the torch expression on the CPU.
    -> y [n, V] f32 (and, on request, the greedy pick's first stage: (values [n, S], indices [n, S] i32), the maximum of each of the S slices of a
    processed row and the first index that holds it)."""
    _need(logits, dtype=torch.float32, name="logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("penalize: logits must be [n, vocab] with contiguous rows")
    n, V = logits.shape
    _need(counts, dtype=None, name="counts")
    if counts.dtype not in (torch.int16, torch.uint16) or counts.dim() != 2 or counts.shape[0] != n or counts.shape[1] < V or counts.stride(1) != 1:
        raise ValueError(f"penalize: counts must be [{n}, >= {V}] int16 / uint16 with contiguous rows")
    for name, t, dt in (("repetition", repetition, torch.float32), ("presence", presence, torch.float32), ("frequency", frequency, torch.float32)) + \
            ((("token", token, torch.int64),) if token is not None else ()):
        _need(t, dtype=dt, name=name)
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"penalize: {name} must be a contiguous tensor of {n} entries")
    import ctypes as C
    lib = _lib.load()
    out = torch.empty((n, V), device=logits.device, dtype=torch.float32)
    S = int(lib.vila_logits_penalize_slices())
    pv = torch.empty((n, S), device=logits.device, dtype=torch.float32) if return_pick else None
    pi = torch.empty((n, S), device=logits.device, dtype=torch.int32) if return_pick else None
    pen = _lib.VilaPenalties(repetition.data_ptr(), presence.data_ptr(), frequency.data_ptr(), counts.data_ptr(), counts.stride(0))
    check(lib.vila_logits_penalize_f32(logits.data_ptr(), logits.stride(0), n, V, C.byref(pen), _p(token), out.data_ptr(), out.stride(0), _p(pv), _p(pi),
                                       _stream()), "penalize")
    return (out, pv, pi) if return_pick else out


LOGPROBS_MAX_TOP = 20


def logits_constrain(logits: torch.Tensor, state: torch.Tensor, cls: torch.Tensor, next: torch.Tensor, n_classes: torch.Tensor,
                     token: Optional[torch.Tensor] = None, return_pick: bool = False, out: Optional[torch.Tensor] = None):
    """Structured output on logits [n, V] fp32 (rows may be strided): the launches the constrained decode steps run between the (penalised) logits and
    the pick.  Row r carries an automaton over token classes (`vila_amd.constrain`): state [n] i32 (device, UPDATED IN PLACE; -1 = the row is
    unconstrained), cls [n, >= V] int16 / uint16 (the bits of uint16 classes; rows may be strided), next [n, ld] int16 (the row's table, row-major
    [states][n_classes[r]], an entry < 0 = not allowed), n_classes [n] i32.  token [n] i64 (optional): the token each row consumes — where it lies
    in 0 .. V - 1 and next[r][s * C + cls[r][t]] >= 0 that entry becomes the row's state first; otherwise the state stays.
    y[r, i] = x[r, i] where next[r][state * C + cls[r][i]] >= 0, else -inf; an unconstrained row returns x's bits.  out: the tensor to write (it may
    be `logits` itself).  The caller binds the device contents: states and classes must lie inside the table.
    -> y [n, V] f32 (and, on request, the greedy pick's first stage as `penalize` returns it; an all -inf row merges to index 0)."""
    _need(logits, dtype=torch.float32, name="logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits_constrain: logits must be [n, vocab] with contiguous rows")
    n, V = logits.shape
    for name, t, dts in (("cls", cls, (torch.int16, torch.uint16)), ("next", next, (torch.int16,))):
        _need(t, dtype=None, name=name)
        if t.dtype not in dts or t.dim() != 2 or t.shape[0] != n or t.stride(1) != 1 or t.shape[1] < 1:
            raise ValueError(f"logits_constrain: {name} must be [{n}, *] {' / '.join(str(d) for d in dts)} with contiguous rows")
    if cls.shape[1] < V:
        raise ValueError(f"logits_constrain: cls must hold at least {V} entries per row")
    for name, t, dt in (("state", state, torch.int32), ("n_classes", n_classes, torch.int32)) + ((("token", token, torch.int64),) if token is not None else ()):
        _need(t, dtype=dt, name=name)
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"logits_constrain: {name} must be a contiguous tensor of {n} entries")
    if out is None:
        out = torch.empty((n, V), device=logits.device, dtype=torch.float32)
    else:
        _need(out, dtype=torch.float32, name="out")
        if out.dim() != 2 or out.shape != logits.shape or out.stride(1) != 1:
            raise ValueError("logits_constrain: out must be [n, vocab] fp32 with contiguous rows")
    import ctypes as C
    lib = _lib.load()
    S = int(lib.vila_logits_constrain_slices())
    pv = torch.empty((n, S), device=logits.device, dtype=torch.float32) if return_pick else None
    pi = torch.empty((n, S), device=logits.device, dtype=torch.int32) if return_pick else None
    con = _lib.VilaConstraints(state.data_ptr(), cls.data_ptr(), cls.stride(0) if n > 1 else cls.shape[1], next.data_ptr(),
                               next.stride(0) if n > 1 else next.shape[1], n_classes.data_ptr())
    check(lib.vila_logits_constrain_f32(logits.data_ptr(), logits.stride(0) if n > 1 else max(logits.stride(0), V), n, V, C.byref(con), _p(token),
                                        out.data_ptr(), out.stride(0) if n > 1 else max(out.stride(0), V), _p(pv), _p(pi), _stream()), "logits_constrain")
    return (out, pv, pi) if return_pick else out


def logprobs(logits: torch.Tensor, token: torch.Tensor, top_n: int = 0):
    """Log-probabilities from RAW logits [n, V] fp32 (rows may be strided; n is not limited to 16): for every row the logprob of token[r] (i64,
    device) and the top_n (0..20) most likely ids with theirs, descending, ties towards the lower index.  logprob(t) = x_t - logsumexp(x), all fp32, in
    a fixed order (the same bits on every run, whatever n).  A token outside 0 .. V - 1 gives NaN; places beyond V hold id -1 / -inf.  The eager form
    of the launch a session opened with logprobs=True runs behind its step.
    -> (token_logprob [n] f32, top_logprob [n, top_n] f32, top_id [n, top_n] i32)."""
    _need(logits, dtype=torch.float32, name="logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logprobs: logits must be [n, vocab] with contiguous rows")
    n, V = logits.shape
    _need(token, dtype=torch.int64, name="token")
    if token.numel() != n or not token.is_contiguous():
        raise ValueError(f"logprobs: token must be a contiguous tensor of {n} entries")
    if isinstance(top_n, bool) or not isinstance(top_n, int) or not 0 <= top_n <= LOGPROBS_MAX_TOP:
        raise ValueError(f"logprobs: top_n must be an integer in 0..{LOGPROBS_MAX_TOP} (got {top_n!r})")
    import ctypes as C
    lib = _lib.load()
    dev = logits.device
    tok_lp = torch.empty((n, 1), device=dev, dtype=torch.float32)
    top_lp = torch.empty((n, 1, LOGPROBS_MAX_TOP), device=dev, dtype=torch.float32) if top_n else None
    top_id = torch.empty((n, 1, LOGPROBS_MAX_TOP), device=dev, dtype=torch.int32) if top_n else None
    ws = torch.empty((lib.vila_logprobs_workspace_bytes(n),), device=dev, dtype=torch.uint8)
    out = _lib.VilaLogprobOut(tok_lp.data_ptr(), _p(top_lp), _p(top_id), 1)
    check(lib.vila_logprobs_f32(logits.data_ptr(), logits.stride(0), n, V, token.data_ptr(), top_n, None, 0, C.byref(out), ws.data_ptr(), _stream()),
          "logprobs")
    if not top_n:
        return tok_lp[:, 0], torch.empty((n, 0), device=dev, dtype=torch.float32), torch.empty((n, 0), device=dev, dtype=torch.int32)
    return tok_lp[:, 0], top_lp[:, 0, :top_n], top_id[:, 0, :top_n]


def _verify_rows(what: str, logits: torch.Tensor, token: torch.Tensor, out: Optional[torch.Tensor]):
    """The shared argument checks of the verify-form operators -> (n, V, out, pv, pi)."""
    _need(logits, dtype=torch.float32, name="logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError(f"{what}: logits must be [n, vocab] with contiguous rows")
    n, V = logits.shape
    _need(token, dtype=torch.int64, name="token")
    if token.numel() != n or not token.is_contiguous():
        raise ValueError(f"{what}: token must be a contiguous tensor of {n} entries")
    if out is None:
        out = torch.empty((n, V), device=logits.device, dtype=torch.float32)
    else:
        _need(out, dtype=torch.float32, name="out")
        if out.dim() != 2 or out.shape != logits.shape or out.stride(1) != 1:
            raise ValueError(f"{what}: out must be [n, vocab] fp32 with contiguous rows")
    S = int(_lib.load().vila_logits_penalize_slices())
    return n, V, out, torch.empty((n, S), device=logits.device, dtype=torch.float32), torch.empty((n, S), device=logits.device, dtype=torch.int32)


def penalize_verify(logits: torch.Tensor, counts: torch.Tensor, repetition: torch.Tensor, presence: torch.Tensor, frequency: torch.Tensor,
                    token: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The penalty launch of the processed verify step: logits [n, V] fp32 are n <= 16 rows of ONE sequence, row i consuming token[i] behind
    token[0 .. i - 1].  counts [>= V] int16 / uint16 (ONE row, only read); repetition / presence / frequency: device tensors of ONE entry.  Row i is
    penalised with min(65535, counts[v] + #{j <= i : token[j] == v}), by `penalize`'s expression.
    -> (y [n, V], pair values [n, S], pair indices [n, S] i32)."""
    n, V, out, pv, pi = _verify_rows("penalize_verify", logits, token, out)
    _need(counts, dtype=None, name="counts")
    if counts.dtype not in (torch.int16, torch.uint16) or counts.dim() != 1 or counts.numel() < V or not counts.is_contiguous():
        raise ValueError(f"penalize_verify: counts must be ONE contiguous row of >= {V} int16 / uint16 entries")
    for name, t in (("repetition", repetition), ("presence", presence), ("frequency", frequency)):
        _need(t, dtype=torch.float32, name=name)
        if t.numel() != 1:
            raise ValueError(f"penalize_verify: {name} must hold ONE entry")
    import ctypes as C
    pen = _lib.VilaPenalties(repetition.data_ptr(), presence.data_ptr(), frequency.data_ptr(), counts.data_ptr(), counts.numel())
    check(_lib.load().vila_logits_penalize_verify_f32(logits.data_ptr(), max(logits.stride(0), V), n, V, C.byref(pen), token.data_ptr(), out.data_ptr(),
                                                      max(out.stride(0), V), pv.data_ptr(), pi.data_ptr(), _stream()), "penalize_verify")
    return out, pv, pi


def constrain_verify(logits: torch.Tensor, state: torch.Tensor, cls: torch.Tensor, next: torch.Tensor, n_classes: torch.Tensor, token: torch.Tensor,
                     out: Optional[torch.Tensor] = None):
    """The automaton launches of the processed verify step: logits [n, V] fp32 are n <= 16 rows of ONE sequence under ONE automaton — state [1] i32
    (only read), cls [>= V] int16 / uint16, next [ld] int16, n_classes [1] i32.  s_0 = adv(state, token[0]), s_i = adv(s_{i-1}, token[i]) by
    `logits_constrain`'s advance rule; row i is masked from s_i.  out may be `logits` itself.
    -> (y [n, V], states [n] i32, pair values [n, S], pair indices [n, S] i32)."""
    n, V, out, pv, pi = _verify_rows("constrain_verify", logits, token, out)
    for name, t, dts, m in (("cls", cls, (torch.int16, torch.uint16), V), ("next", next, (torch.int16,), 1)):
        _need(t, dtype=None, name=name)
        if t.dtype not in dts or t.dim() != 1 or t.numel() < m or not t.is_contiguous():
            raise ValueError(f"constrain_verify: {name} must be ONE contiguous row of >= {m} entries")
    for name, t in (("state", state), ("n_classes", n_classes)):
        _need(t, dtype=torch.int32, name=name)
        if t.numel() != 1:
            raise ValueError(f"constrain_verify: {name} must hold ONE entry")
    import ctypes as C
    states = torch.empty(n, device=logits.device, dtype=torch.int32)
    con = _lib.VilaConstraints(state.data_ptr(), cls.data_ptr(), cls.numel(), next.data_ptr(), next.numel(), n_classes.data_ptr())
    check(_lib.load().vila_logits_constrain_verify_f32(logits.data_ptr(), max(logits.stride(0), V), n, V, C.byref(con), token.data_ptr(), states.data_ptr(),
                                                       out.data_ptr(), max(out.stride(0), V), pv.data_ptr(), pi.data_ptr(), _stream()), "constrain_verify")
    return out, states, pv, pi


def verify_commit(vocab: int, consumed: torch.Tensor, n_accept: torch.Tensor, counts: Optional[torch.Tensor] = None,
                  state: Optional[torch.Tensor] = None, states: Optional[torch.Tensor] = None) -> None:
    """The commit behind a verify step's accept, in place: with m = n_accept[0] (i32, device; clamped to 0 .. n - 1), counts [>= vocab] (ONE row) gets
    one saturating bump for each of consumed[0 .. m] (i64 [n]; ids outside the vocabulary bump nothing) and state [1] i32 becomes states[m]."""
    _need(consumed, dtype=torch.int64, name="consumed")
    _need(n_accept, dtype=torch.int32, name="n_accept")
    n = consumed.numel()
    if counts is not None and (counts.dtype not in (torch.int16, torch.uint16) or counts.dim() != 1 or counts.numel() < vocab or not counts.is_contiguous()):
        raise ValueError(f"verify_commit: counts must be ONE contiguous row of >= {vocab} int16 / uint16 entries")
    if (state is None) != (states is None) or (states is not None and (states.dtype != torch.int32 or states.numel() != n or state.dtype != torch.int32)):
        raise ValueError(f"verify_commit: state [1] i32 comes with states [{n}] i32")
    import ctypes as C
    pen = None if counts is None else _lib.VilaPenalties(counts.data_ptr(), counts.data_ptr(), counts.data_ptr(), counts.data_ptr(), counts.numel())
    con = None if state is None else _lib.VilaConstraints(state.data_ptr(), None, 0, None, 0, None)
    check(_lib.load().vila_verify_commit(None if pen is None else C.byref(pen), None if con is None else C.byref(con), int(vocab), consumed.data_ptr(),
                                         _p(states), n_accept.data_ptr(), n, _stream()), "verify_commit")


def logprobs_seq(logits: torch.Tensor, token: torch.Tensor, rec: torch.Tensor, token_lp: torch.Tensor, top_lp: torch.Tensor, top_id: torch.Tensor) -> None:
    """`logprobs` for the rows of ONE sequence, in place: row r of logits [n, V] writes record rec[r] (i32, device; outside 0 .. max_rec - 1: nothing) of
    token_lp [max_rec] f32, top_lp [max_rec, 20] f32 and top_id [max_rec, 20] i32 — what the processed verify step runs behind its accept."""
    _need(logits, dtype=torch.float32, name="logits")
    n, V = logits.shape
    _need(token, dtype=torch.int64, name="token")
    _need(rec, dtype=torch.int32, name="rec")
    max_rec = token_lp.numel()
    if token.numel() != n or rec.numel() != n or tuple(top_lp.shape) != (max_rec, LOGPROBS_MAX_TOP) or tuple(top_id.shape) != (max_rec, LOGPROBS_MAX_TOP) or \
            token_lp.dtype != torch.float32 or top_lp.dtype != torch.float32 or top_id.dtype != torch.int32 or \
            not (token_lp.is_contiguous() and top_lp.is_contiguous() and top_id.is_contiguous()):
        raise ValueError(f"logprobs_seq: token / rec hold {n} entries, token_lp [max_rec] f32, top_lp / top_id [max_rec, {LOGPROBS_MAX_TOP}] f32 / i32, contiguous")
    import ctypes as C
    lib = _lib.load()
    ws = torch.empty((lib.vila_logprobs_workspace_bytes(n),), device=logits.device, dtype=torch.uint8)
    out = _lib.VilaLogprobOut(token_lp.data_ptr(), top_lp.data_ptr(), top_id.data_ptr(), max_rec)
    check(lib.vila_logprobs_seq_f32(logits.data_ptr(), logits.stride(0), n, V, token.data_ptr(), LOGPROBS_MAX_TOP, rec.data_ptr(), C.byref(out), ws.data_ptr(),
                                    _stream()), "logprobs_seq")


def attn_decode_batch(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, pos: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """The batched decode step's attention on its own: q [n, q_heads, 128] bf16 (rows may be strided), kcache / vcache ONE layer's
    [slots >= n, kv_heads, max_ctx, 128] bf16 (contiguous), pos [n] i32 — row i attends keys 0 .. pos[i] of slot i.  max_ctx up to 32768, GQA
    groups of 1, 2, 4, 7 or 8; the kernel form is chosen as the step chooses it (`vila_decode_batch_force_slices`).  -> o [n, q_heads, 128]."""
    _need(q, name="q"); _need(kcache, name="kcache"); _need(vcache, name="vcache"); _need(pos, dtype=torch.int32, name="pos")
    if q.dim() != 3 or q.shape[2] != 128 or q.stride(2) != 1 or q.stride(1) != 128:
        raise ValueError("attn_decode_batch: q must be [n, q_heads, 128] with contiguous heads")
    n, nq, _ = q.shape
    if kcache.dim() != 4 or kcache.shape != vcache.shape or kcache.shape[3] != 128 or not kcache.is_contiguous() or not vcache.is_contiguous():
        raise ValueError("attn_decode_batch: kcache / vcache must be contiguous [slots, kv_heads, max_ctx, 128] of one shape")
    slots, nkv, max_ctx, _ = kcache.shape
    if slots < n or pos.numel() != n or not pos.is_contiguous():
        raise ValueError(f"attn_decode_batch: {n} rows need {n} cache slots and {n} contiguous positions")
    lib = _lib.load()
    o = torch.empty((n, nq, 128), device=q.device, dtype=torch.bfloat16)
    ws = torch.empty((lib.vila_attn_decode_batch_workspace_bytes(n, nq, max_ctx),), device=q.device, dtype=torch.uint8)
    check(lib.vila_attn_decode_batch_bf16(q.data_ptr(), q.stride(0), kcache.data_ptr(), vcache.data_ptr(), kcache.stride(0), pos.data_ptr(), o.data_ptr(),
                                          o.stride(0), n, nq, nkv, max_ctx, float(scale if scale is not None else 128 ** -0.5), ws.data_ptr(), ws.numel(),
                                          _stream()), "attn_decode_batch")
    return o


def attn_decode_batch_prefix(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, pos: torch.Tensor, shared_len: torch.Tensor, uses: torch.Tensor,
                             prefix_slot: Optional[int] = None, shared_len_host: Optional[int] = None, scale: Optional[float] = None) -> torch.Tensor:
    """The attention of a batch session with a shared prompt prefix, on its own: `attn_decode_batch`'s operands with one slot more in the cache, the
    prefix slot (default: the last).  shared_len: device int32 scalar S, a multiple of 256; uses [n] i32.  Row i with uses[i] != 0 attends keys
    0 .. S - 1 of the prefix slot and keys S .. pos[i] of slot i (pos[i] >= S); a row with uses[i] == 0 attends keys 0 .. pos[i] of slot i, with the
    bits of `attn_decode_batch` in walking form.  shared_len_host: S where the host knows it (checked), else left to the device.  n <= 16.
    -> o [n, q_heads, 128]."""
    _need(q, name="q"); _need(kcache, name="kcache"); _need(vcache, name="vcache"); _need(pos, dtype=torch.int32, name="pos")
    _need(shared_len, dtype=torch.int32, name="shared_len"); _need(uses, dtype=torch.int32, name="uses")
    if q.dim() != 3 or q.shape[2] != 128 or q.stride(2) != 1 or q.stride(1) != 128:
        raise ValueError("attn_decode_batch_prefix: q must be [n, q_heads, 128] with contiguous heads")
    n, nq, _ = q.shape
    if kcache.dim() != 4 or kcache.shape != vcache.shape or kcache.shape[3] != 128 or not kcache.is_contiguous() or not vcache.is_contiguous():
        raise ValueError("attn_decode_batch_prefix: kcache / vcache must be contiguous [slots, kv_heads, max_ctx, 128] of one shape")
    slots, nkv, max_ctx, _ = kcache.shape
    if pos.numel() != n or not pos.is_contiguous() or uses.numel() != n or not uses.is_contiguous() or shared_len.numel() != 1:
        raise ValueError(f"attn_decode_batch_prefix: {n} rows need {n} contiguous positions and flags and one shared length")
    lib = _lib.load()
    o = torch.empty((n, nq, 128), device=q.device, dtype=torch.bfloat16)
    ws = torch.empty((lib.vila_attn_decode_batch_prefix_workspace_bytes(n, nq, max_ctx),), device=q.device, dtype=torch.uint8)
    check(lib.vila_attn_decode_batch_prefix_bf16(q.data_ptr(), q.stride(0), kcache.data_ptr(), vcache.data_ptr(), kcache.stride(0), slots,
                                                 slots - 1 if prefix_slot is None else int(prefix_slot), shared_len.data_ptr(),
                                                 -1 if shared_len_host is None else int(shared_len_host), uses.data_ptr(), pos.data_ptr(), o.data_ptr(),
                                                 o.stride(0), n, nq, nkv, max_ctx, float(scale if scale is not None else 128 ** -0.5), ws.data_ptr(),
                                                 ws.numel(), _stream()), "attn_decode_batch_prefix")
    return o


def attn_append(q: torch.Tensor, kslot: torch.Tensor, vslot: torch.Tensor, past: int, scale: Optional[float] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal attention with a key prefix (the append prefill's attention on its own): q [T, q_heads, 128] bf16 (rows may be strided) at positions
    past .. past + T - 1 of ONE sequence; kslot / vslot one layer's slot [kv_heads, max_ctx, 128] bf16 (contiguous) holding the keys / values of
    positions 0 .. past + T - 1.  Row i attends keys 0 .. past + i; rows of the slot at or beyond past + T are never read.  The block form follows
    `vila_attn_force_append`.  -> o [T, q_heads, 128] (`out`, if given, is written and returned)."""
    _need(q, name="q"); _need(kslot, name="kslot"); _need(vslot, name="vslot")
    if q.dim() != 3 or q.shape[2] != 128 or q.stride(2) != 1 or q.stride(1) != 128:
        raise ValueError("attn_append: q must be [T, q_heads, 128] with contiguous heads")
    T, nq, _ = q.shape
    if kslot.dim() != 3 or kslot.shape != vslot.shape or kslot.shape[2] != 128 or not kslot.is_contiguous() or not vslot.is_contiguous():
        raise ValueError("attn_append: kslot / vslot must be contiguous [kv_heads, max_ctx, 128] of one shape")
    nkv, max_ctx, _ = kslot.shape
    past = int(past)
    if past < 0 or T < 1 or past + T > max_ctx:
        raise ValueError(f"attn_append: past ({past}) >= 0, T ({T}) >= 1 and past + T <= max_ctx ({max_ctx}) are required")
    o = torch.empty((T, nq, 128), device=q.device, dtype=torch.bfloat16) if out is None else out
    if out is not None:
        _need(out, name="out")
        if out.shape != (T, nq, 128) or out.stride(2) != 1 or out.stride(1) != 128:
            raise ValueError("attn_append: out must be [T, q_heads, 128] with contiguous heads")
    check(_lib.load().vila_attn_append_bf16(q.data_ptr(), q.stride(0), kslot.data_ptr(), vslot.data_ptr(), past, T, o.data_ptr(), o.stride(0), nq, nkv,
                                            max_ctx, float(scale if scale is not None else 128 ** -0.5), _stream()), "attn_append")
    return o


def attn_decode_verify(q: torch.Tensor, kslot: torch.Tensor, vslot: torch.Tensor, pos: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """The verify step's attention on its own: q [n, q_heads, 128] bf16 (rows may be strided), n in 1..16 consecutive positions of ONE sequence;
    kslot / vslot one layer's slot [kv_heads, max_ctx, 128] bf16 (contiguous); pos a device int32 scalar — row i attends keys
    0 .. min(pos + i, max_ctx - 1), and the slot's K/V is read once for all rows.  GQA groups of 1, 2, 4, 7 or 8; the slice count follows
    `vila_decode_batch_force_slices`.  -> o [n, q_heads, 128]."""
    _need(q, name="q"); _need(kslot, name="kslot"); _need(vslot, name="vslot"); _need(pos, dtype=torch.int32, name="pos")
    if q.dim() != 3 or q.shape[2] != 128 or q.stride(2) != 1 or q.stride(1) != 128:
        raise ValueError("attn_decode_verify: q must be [n, q_heads, 128] with contiguous heads")
    n, nq, _ = q.shape
    if kslot.dim() != 3 or kslot.shape != vslot.shape or kslot.shape[2] != 128 or not kslot.is_contiguous() or not vslot.is_contiguous():
        raise ValueError("attn_decode_verify: kslot / vslot must be contiguous [kv_heads, max_ctx, 128] of one shape")
    nkv, max_ctx, _ = kslot.shape
    if pos.numel() != 1:
        raise ValueError("attn_decode_verify: pos is one device scalar, the position of row 0")
    lib = _lib.load()
    o = torch.empty((n, nq, 128), device=q.device, dtype=torch.bfloat16)
    ws = torch.empty((lib.vila_attn_decode_verify_workspace_bytes(n, nq, max_ctx),), device=q.device, dtype=torch.uint8)
    check(lib.vila_attn_decode_verify_bf16(q.data_ptr(), q.stride(0), kslot.data_ptr(), vslot.data_ptr(), pos.data_ptr(), o.data_ptr(), o.stride(0), n, nq, nkv,
                                           max_ctx, float(scale if scale is not None else 128 ** -0.5), ws.data_ptr(), ws.numel(), _stream()),
          "attn_decode_verify")
    return o


ATTN_DECODE_FORMS = {"head": 0, "slices256": 1, "split64": 2}


def attn_decode(q: torch.Tensor, kslot: torch.Tensor, vslot: torch.Tensor, pos: torch.Tensor, form: str = "head", scale: Optional[float] = None,
                w=None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The batch-1 decode step's attention on its own: q [q_heads, 128] bf16, kslot / vslot one layer's slot [kv_heads, max_ctx, 128] bf16
    (contiguous), pos a device int32 scalar below max_ctx — keys 0 .. pos are attended.  GQA groups of 1..8.  form: "head" (one block per query
    head, max_ctx <= 2048) or "split64" (64-key split-KV + merge launch, max_ctx > 2048) -> o [q_heads, 128]; "slices256" (the step's default up
    to 2048 positions: 256-key slices merged in the o_proj GEMV's prologue) needs the o_proj weight `w`, bf16 [N, q_heads * 128] or a
    vila_amd.quant.W4Matrix -> y [N] = w . o (+ residual [N]).  The kernels read pos + 1 keys unguarded, so a position at or past the capacity is
    refused here (one host read of pos)."""
    _need(q, name="q"); _need(kslot, name="kslot"); _need(vslot, name="vslot"); _need(pos, dtype=torch.int32, name="pos")
    if form not in ATTN_DECODE_FORMS:
        raise ValueError(f"attn_decode: form must be one of {sorted(ATTN_DECODE_FORMS)}, got {form!r}")
    if q.dim() != 2 or q.shape[1] != 128 or not q.is_contiguous():
        raise ValueError("attn_decode: q must be contiguous [q_heads, 128]")
    nq = q.shape[0]
    if kslot.dim() != 3 or kslot.shape != vslot.shape or kslot.shape[2] != 128 or not kslot.is_contiguous() or not vslot.is_contiguous():
        raise ValueError("attn_decode: kslot / vslot must be contiguous [kv_heads, max_ctx, 128] of one shape")
    nkv, max_ctx, _ = kslot.shape
    if pos.numel() != 1:
        raise ValueError("attn_decode: pos is one device scalar")
    p = int(pos)
    if not 0 <= p < max_ctx:
        raise ValueError(f"attn_decode: position {p} outside the cache of {max_ctx} positions")
    if (form == "slices256") != (w is not None):
        raise ValueError("attn_decode: the o_proj weight goes with form 'slices256', and only with it")
    lib = _lib.load()
    sc = float(scale if scale is not None else 128 ** -0.5)
    ws = torch.empty((lib.vila_attn_decode_workspace_bytes(nq, max_ctx),), device=q.device, dtype=torch.uint8)
    if w is None:
        o = torch.empty((nq, 128), device=q.device, dtype=torch.bfloat16)
        check(lib.vila_attn_decode_bf16(q.data_ptr(), kslot.data_ptr(), vslot.data_ptr(), pos.data_ptr(), o.data_ptr(), nq, nkv, max_ctx, sc,
                                        ATTN_DECODE_FORMS[form], ws.data_ptr(), ws.numel(), _stream()), "attn_decode")
        return o
    if residual is not None:
        _need(residual, name="residual")
    if isinstance(w, torch.Tensor):
        _need(w, name="w")
        if w.dim() != 2 or w.shape[1] != nq * 128 or not w.is_contiguous():
            raise ValueError(f"attn_decode: w must be contiguous [N, {nq * 128}]")
        N = w.shape[0]
        if residual is not None and residual.numel() != N:
            raise ValueError(f"attn_decode: residual must have {N} entries")
        y = torch.empty((N,), device=q.device, dtype=torch.bfloat16)
        check(lib.vila_attn_decode_oproj_bf16(q.data_ptr(), kslot.data_ptr(), vslot.data_ptr(), pos.data_ptr(), w.data_ptr(), _p(residual), y.data_ptr(), N,
                                              nq, nkv, max_ctx, sc, ws.data_ptr(), ws.numel(), _stream()), "attn_decode_oproj")
        return y
    _need(w.q, dtype=torch.int32, name="w.q"); _need(w.sz, dtype=torch.int32, name="w.sz")
    if w.K != nq * 128 or w.mode != 0:
        raise ValueError(f"attn_decode: the W4 matrix must be a plain one with K = {nq * 128} (got K = {w.K}, mode {w.mode})")
    if residual is not None and residual.numel() != w.N:
        raise ValueError(f"attn_decode: residual must have {w.N} entries")
    y = torch.empty((w.N,), device=q.device, dtype=torch.bfloat16)
    check(lib.vila_attn_decode_oproj_w4(q.data_ptr(), kslot.data_ptr(), vslot.data_ptr(), pos.data_ptr(), w.q.data_ptr(), w.sz.data_ptr(), _p(residual),
                                        y.data_ptr(), w.N, nq, nkv, max_ctx, sc, ws.data_ptr(), ws.numel(), _stream()), "attn_decode_oproj_w4")
    return y


def prompt_lookup_draft(hist: torch.Tensor, n_hist: int, k: int, max_ngram: int = 2) -> list:
    """The verify step's draft stage on its own: hist int64 on the device, the first n_hist ids are the history -> up to k draft ids (a list),
    what `host.prompt_lookup_draft(hist[:n_hist], k, max_ngram)` returns."""
    _need(hist, dtype=torch.int64, name="hist")
    if not 1 <= k <= 15 or not 1 <= n_hist <= hist.numel() or max_ngram < 1:
        raise ValueError("prompt_lookup_draft: k in 1..15, 1 <= n_hist <= len(hist), max_ngram >= 1")
    nh = torch.full((1,), int(n_hist), device=hist.device, dtype=torch.int32)
    token = torch.full((k + 1,), -1, device=hist.device, dtype=torch.int64)
    nd = torch.zeros(1, device=hist.device, dtype=torch.int32)
    check(_lib.load().vila_prompt_lookup_draft(hist.data_ptr(), nh.data_ptr(), int(max_ngram), k + 1, token.data_ptr(), nd.data_ptr(), _stream()),
          "prompt_lookup_draft")
    return token[1:1 + int(nd.item())].tolist()


def embed_tokens(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    _need(table, name="embed table")
    ids = ids.to(device=table.device, dtype=torch.int64).contiguous()
    out = torch.empty((*ids.shape, table.shape[1]), device=table.device, dtype=table.dtype)
    check(_lib.load().vila_embed_tokens(table.data_ptr(), table.shape[0], table.shape[1], ids.data_ptr(), ids.numel(),
                                        out.data_ptr(), _stream()), "embed_tokens")
    return out


def copy_rows(src: torch.Tensor, dst: torch.Tensor, src_row: Optional[torch.Tensor], dst_row: Optional[torch.Tensor], n: int) -> None:
    _need(src, name="src"); _need(dst, name="dst")
    for t in (src_row, dst_row):
        assert t is None or (t.dtype == torch.int32 and t.is_cuda)
    check(_lib.load().vila_copy_rows(src.data_ptr(), dst.data_ptr(), _p(src_row), _p(dst_row), n, src.shape[-1], _stream()), "copy_rows")


def quant_rows_i8(x: torch.Tensor):
    """bf16 [rows, cols] -> (int8 [rows, cols], fp32 scale [rows]): per-token dynamic symmetric quantisation (scale = max|row| / 127)."""
    _need(x, name="x")
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    q = torch.empty(x2.shape, device=x.device, dtype=torch.int8)
    sc = torch.empty((x2.shape[0],), device=x.device, dtype=torch.float32)
    check(_lib.load().vila_quant_rows_i8(x2.data_ptr(), q.data_ptr(), sc.data_ptr(), x2.shape[0], x2.shape[1], _stream()), "quant_rows_i8")
    return q, sc


def gemm_w8a8(aq: torch.Tensor, sx: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, bias: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, epi: int = EPI_NONE) -> torch.Tensor:
    """out[M,N] bf16 = epi((aq[M,K] . wq[N,K]^T) * sx[m] * sw[n] + bias) (+ residual); int8 operands, int32 accumulate."""
    assert aq.dtype == torch.int8 and wq.dtype == torch.int8 and aq.is_cuda and aq.stride(1) == 1 and wq.stride(1) == 1
    M, K = aq.shape
    N = wq.shape[0]
    out = torch.empty((M, N), device=aq.device, dtype=torch.bfloat16)
    check(_lib.load().vila_gemm_w8a8(aq.data_ptr(), aq.stride(0), wq.data_ptr(), wq.stride(0), sx.data_ptr(), sw.data_ptr(), _p(bias), _p(residual),
                                     residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), M, N, K, epi, _stream()),
          "vila_gemm_w8a8")
    return out


def video_pool(feats: torch.Tensor, pool, start_rows: Optional[torch.Tensor] = None, end_rows: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feats [nt, nl*nl, C] (one video's projected frames) -> [(nt/pt) * (n_start + (nl/ph)(nl/pw) + n_end), C]: TSPVideoEncoder's
    pool + _process_features (video/tsp.py:10-11,28-52); pool (1,1,1) = BasicVideoEncoder (video/basic.py:30-41)."""
    _need(feats, name="feats")
    nt, ns, Cc = feats.shape
    nl = int(round(ns ** 0.5))
    assert nl * nl == ns
    pt, ph, pw = (int(p) for p in pool)
    n_s = 0 if start_rows is None else start_rows.shape[0]
    n_e = 0 if end_rows is None else end_rows.shape[0]
    if pt <= 0 or ph <= 0 or pw <= 0 or nt % pt or nl % ph or nl % pw:
        raise ValueError(f"shape '[{nt}, {nl}, {nl}]' is invalid for pooling by ({pt}, {ph}, {pw}): every pooled dimension must divide evenly")
    rows = (nt // pt) * (n_s + (nl // ph) * (nl // pw) + n_e)
    if out is None:
        out = torch.empty((rows, Cc), device=feats.device, dtype=feats.dtype)
    assert out.shape == (rows, Cc) and out.is_contiguous()
    check(_lib.load().vila_video_pool_bf16(feats.contiguous().data_ptr(), out.data_ptr(), nt, nl, Cc, pt, ph, pw,
                                           _p(start_rows.contiguous() if start_rows is not None else None), n_s,
                                           _p(end_rows.contiguous() if end_rows is not None else None), n_e, _stream()), "video_pool")
    return out


def video_pool_bwd(dpooled: torch.Tensor, nt: int, nl: int, pool, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """Adjoint of video_pool's feature rows: dpooled [(nt/pt)(nl/ph)(nl/pw), C] -> dfeats [nt, nl*nl, C] (the `mean` backward of tsp.py:10-11);
    accumulate adds into `out` (the later pool sizes of one video)."""
    _need(dpooled, name="dpooled")
    pt, ph, pw = (int(p) for p in pool)
    Cc = dpooled.shape[-1]
    assert dpooled.is_contiguous() and dpooled.numel() == (nt // pt) * (nl // ph) * (nl // pw) * Cc
    if out is None:
        assert not accumulate
        out = torch.empty((nt, nl * nl, Cc), device=dpooled.device, dtype=dpooled.dtype)
    assert out.is_contiguous() and out.numel() == nt * nl * nl * Cc
    check(_lib.load().vila_video_pool_bwd_bf16(dpooled.data_ptr(), out.data_ptr(), nt, nl, Cc, pt, ph, pw, int(accumulate), _stream()), "video_pool_bwd")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# SFT-step operators (backward + optimizer)
# ----------------------------------------------------------------------------------------------------------------------
def _L():
    return _lib.load()


def transpose(x: torch.Tensor) -> torch.Tensor:
    """[R, C] -> [C, round_up(R, 64)] (zero-padded): the K-contiguous operand form gemm() needs for dgrad / wgrad
    (64 = the K-tile of the 256x256 kernel, so the padded token dimension never needs a K tail)."""
    _need(x, name="x"); assert x.dim() == 2 and x.stride(1) == 1
    R, Cc = x.shape
    Rp = (R + 63) // 64 * 64
    out = torch.empty((Cc, Rp), device=x.device, dtype=x.dtype)
    check(_L().vila_transpose_bf16(x.data_ptr(), out.data_ptr(), R, Cc, x.stride(0), Rp, _stream()), "transpose")
    return out


def act_fwd(z: torch.Tensor, act: int) -> torch.Tensor:
    y = torch.empty_like(z)
    check(_L().vila_act_fwd_bf16(z.data_ptr(), y.data_ptr(), z.numel(), act, _stream()), "act_fwd")
    return y


def act_bwd(z: torch.Tensor, dy: torch.Tensor, act: int) -> torch.Tensor:
    dz = torch.empty_like(z)
    check(_L().vila_act_bwd_bf16(z.data_ptr(), dy.data_ptr(), dz.data_ptr(), z.numel(), act, _stream()), "act_bwd")
    return dz


def silu_mul(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    a = torch.empty_like(g)
    check(_L().vila_silu_mul_fwd_bf16(g.data_ptr(), u.data_ptr(), a.data_ptr(), g.numel(), _stream()), "silu_mul")
    return a


def silu_mul_bwd(g, u, da):
    dg, du = torch.empty_like(g), torch.empty_like(u)
    check(_L().vila_silu_mul_bwd_bf16(g.data_ptr(), u.data_ptr(), da.data_ptr(), dg.data_ptr(), du.data_ptr(), g.numel(), _stream()), "silu_mul_bwd")
    return dg, du


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty_like(a) if out is None else out
    check(_L().vila_add_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "add")
    return out


def grad_accum(acc: torch.Tensor, g: torch.Tensor, out: Optional[torch.Tensor] = None, mode: int = 1) -> None:
    """Gradient accumulation in fp32 (vila_grad_accum_f32): mode 0 acc = g, 1 acc += g, 2 out = bf16(acc + g)."""
    assert acc.dtype == torch.float32 and g.dtype == torch.bfloat16 and acc.numel() == g.numel() and acc.is_contiguous() and g.is_contiguous()
    assert int(mode) in (0, 1, 2) and g.numel() % 8 == 0, (mode, g.numel())
    if int(mode) == 2:       # a mode-2 call without (or with a mis-shaped) output used to be caught only inside the library
        assert out is not None and out.dtype == torch.bfloat16 and out.numel() == g.numel() and out.is_contiguous() and out.device == g.device
    check(_L().vila_grad_accum_f32(acc.data_ptr(), g.data_ptr(), _p(out), g.numel(), int(mode), _stream()), "grad_accum")


def colsum(x: torch.Tensor, out: torch.Tensor, accumulate: bool = False, period: int = 0) -> None:
    assert x.dim() == 2 and x.stride(1) == 1 and out.is_contiguous()
    scratch = torch.empty((int(_L().vila_colsum_scratch_floats(x.shape[0], x.shape[1])),), device=x.device, dtype=torch.float32) if period == 0 else None
    check(_L().vila_colsum_bf16(x.data_ptr(), out.data_ptr(), _p(scratch), x.shape[0], x.shape[1], x.stride(0), int(accumulate), period, _stream()), "colsum")


def norm_bwd(x, w, dy, dw_out, db_out, eps: float, rms: bool, accumulate: bool = False) -> torch.Tensor:
    x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, x.shape[-1])
    dx = torch.empty_like(x2)
    scratch = torch.empty((int(_L().vila_norm_bwd_scratch_floats(x2.shape[0], x2.shape[1])),), device=x.device, dtype=torch.float32)
    check(_L().vila_norm_bwd_bf16(x2.data_ptr(), w.data_ptr(), dy2.data_ptr(), dx.data_ptr(), dw_out.data_ptr(), _p(db_out),
                                  scratch.data_ptr(), x2.shape[0], x2.shape[1], eps, int(rms), int(accumulate), _stream()), "norm_bwd")
    return dx.view(x.shape)


def ce_loss(logits: torch.Tensor, labels: torch.Tensor, loss_acc: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [n, V] fp32, labels [n] i64 -> dlogits [n, V] bf16 (into `out` when given); loss_acc (fp32 scalar on device) += sum CE * scale."""
    _need(logits, dtype=torch.float32, name="logits")
    n, V = logits.shape
    d = torch.empty((n, V), device=logits.device, dtype=torch.bfloat16) if out is None else out
    assert d.shape == (n, V) and d.dtype == torch.bfloat16 and d.is_contiguous() and labels.is_contiguous()
    row_loss = torch.empty((max(n, 1),), device=logits.device, dtype=torch.float32)
    check(_L().vila_ce_loss_f32(logits.data_ptr(), labels.data_ptr(), d.data_ptr(), loss_acc.data_ptr(), row_loss.data_ptr(), n, V, logits.stride(0), scale,
                                _stream()), "ce_loss")
    return d


def scatter_add_rows(src: torch.Tensor, dst: torch.Tensor, rows: torch.Tensor) -> None:
    assert rows.dtype == torch.int32 and src.is_contiguous() and dst.is_contiguous()
    check(_L().vila_scatter_add_rows_bf16(src.data_ptr(), dst.data_ptr(), rows.data_ptr(), rows.numel(), src.shape[-1], _stream()), "scatter_add_rows")


def depth_to_space(dy: torch.Tensor, g: int, k: int) -> torch.Tensor:
    B, _, CC = dy.shape
    Cc = CC // (k * k)
    dx = torch.empty((B, g * g, Cc), device=dy.device, dtype=dy.dtype)
    check(_L().vila_depth_to_space_bf16(dy.contiguous().data_ptr(), dx.data_ptr(), B, g, Cc, k, _stream()), "depth_to_space")
    return dx


def im2col(px: torch.Tensor, patch: int, kp: int) -> torch.Tensor:
    B, Cc, H, W = px.shape
    out = torch.empty((B * (H // patch) * (W // patch), kp), device=px.device, dtype=px.dtype)
    check(_L().vila_im2col_bf16(px.contiguous().data_ptr(), out.data_ptr(), B, Cc, H, W, patch, kp, _stream()), "im2col")
    return out


def rope_table(positions: torch.Tensor, head_dim: int, theta: float):
    S = positions.numel()
    cs = torch.empty((S, head_dim // 2), device=positions.device, dtype=torch.float32)
    sn = torch.empty_like(cs)
    check(_L().vila_rope_table_f32(positions.data_ptr(), cs.data_ptr(), sn.data_ptr(), S, head_dim, theta, _stream()), "rope_table")
    return cs, sn


def rope_fwd_(qkv: torch.Tensor, cs, sn, positions, nq: int, nkv: int, hd: int) -> None:
    check(_L().vila_rope_fwd_bf16(qkv.data_ptr(), cs.data_ptr(), sn.data_ptr(), positions.data_ptr(), qkv.shape[0], nq, nkv, hd, _stream()), "rope_fwd")


def rope_bwd_(dqkv: torch.Tensor, cs, sn, nq: int, nkv: int, hd: int) -> None:
    check(_L().vila_rope_bwd_bf16(dqkv.data_ptr(), cs.data_ptr(), sn.data_ptr(), dqkv.shape[0], nq, nkv, hd, _stream()), "rope_bwd")


def attn_bwd(q, k, v, o, do, lse, causal: bool, dq, dk, dv, scale: Optional[float] = None, cu_seqlens=None, max_seqlen=None, n_seq: int = 1,
             parts: int = 7, delta: Optional[torch.Tensor] = None) -> torch.Tensor:
    """All of q,k,v,o,do,dq,dk,dv are [T, H, D] views (last dim contiguous).  lse [Hq, T] fp32 from attn_fwd(return_lse=True).
    parts (bit mask): 1 = delta = rowsum(dO o O), 2 = dQ, 4 = dK / dV; the default does all three.  Returns delta [Hq, T] fp32, to be
    passed back in when the parts are launched separately (dQ and dK / dV share no output and may run on different streams)."""
    import ctypes as C
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    ts = (C.c_int64 * 8)(*[t.stride(0) for t in (q, k, v, o, do, dq, dk, dv)])
    hs = (C.c_int32 * 8)(*[t.stride(1) for t in (q, k, v, o, do, dq, dk, dv)])
    if cu_seqlens is not None:
        n_seq = cu_seqlens.numel() - 1
    else:
        max_seqlen = T // n_seq
    if delta is None:
        if not parts & 1:
            raise ValueError("attn_bwd: parts without 1 (delta) need the delta tensor of an earlier call")
        delta = torch.empty((Hq, T), device=q.device, dtype=torch.float32)
    check(_L().vila_attn_bwd_bf16_parts(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                        dv.data_ptr(), ts, hs, _p(cu_seqlens), n_seq, T, int(max_seqlen), Hq, Hkv, D, int(causal),
                                        float(scale if scale is not None else D ** -0.5), lse.data_ptr(), delta.data_ptr(), int(parts), _stream()),
          "attn_bwd")
    return delta


def adamw_step(master, m, v, grad, param, lr, beta1, beta2, eps, wd, step: int, grad_scale: float = 1.0, lean: bool = False) -> None:
    """torch.optim.AdamW update on flat buffers.  lean: the <= 32-VGPR kernel that fits beside a resident 256x256 GEMM block (side streams)."""
    if lean:
        check(_L().vila_adamw_step_lean(master.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.data_ptr(), master.numel(), lr, beta1,
                                        beta2, eps, wd, step, grad_scale, _stream()), "adamw_lean")
        return
    check(_L().vila_adamw_step(master.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.data_ptr(), master.numel(), lr, beta1, beta2,
                               eps, wd, step, grad_scale, _stream()), "adamw")


def sumsq(x: torch.Tensor) -> torch.Tensor:
    out = torch.zeros((1,), device=x.device, dtype=torch.float32)
    scratch = torch.empty((2048,), device=x.device, dtype=torch.float32)          # VILA_SUMSQ_SCRATCH_FLOATS
    check(_L().vila_sumsq_bf16(x.data_ptr(), x.numel(), out.data_ptr(), scratch.data_ptr(), _stream()), "sumsq")
    return out


def s2_merge(feats: torch.Tensor, desc: torch.Tensor, n_scales: int, splits) -> torch.Tensor:
    """dynamic_s2: tower output [n_tiles, N, C] + block descriptors [n_blocks, 6] i32 -> projector input [n_blocks, N, n_scales*C]."""
    import ctypes as C
    _need(feats, name="feats")
    assert desc.dtype == torch.int32 and desc.is_cuda and desc.dim() == 2 and desc.shape[1] == 6
    n_tiles, N, Cc = feats.shape
    g = int(round(N ** 0.5))
    out = torch.empty((desc.shape[0], N, n_scales * Cc), device=feats.device, dtype=feats.dtype)
    sp = (C.c_int32 * max(len(splits), 1))(*splits) if len(splits) else (C.c_int32 * 1)(1)
    check(_L().vila_s2_merge_bf16(feats.contiguous().data_ptr(), out.data_ptr(), desc.contiguous().data_ptr(), desc.shape[0], g, Cc, n_scales, sp,
                                  _stream()), "s2_merge")
    return out


def s2_merge_bwd(dy: torch.Tensor, tile_desc: torch.Tensor, n_scales: int, splits) -> torch.Tensor:
    """Adjoint of s2_merge: dy [n_blocks, N, n_scales*C] + per-tile descriptors [n_tiles, 8] i32 (host.s2_plan) -> dfeats [n_tiles, N, C]."""
    import ctypes as C
    _need(dy, name="dy")
    assert tile_desc.dtype == torch.int32 and tile_desc.is_cuda and tile_desc.dim() == 2 and tile_desc.shape[1] == 8
    _, N, CC = dy.shape
    Cc = CC // n_scales
    g = int(round(N ** 0.5))
    dx = torch.empty((tile_desc.shape[0], N, Cc), device=dy.device, dtype=dy.dtype)
    sp = (C.c_int32 * max(len(splits), 1))(*splits) if len(splits) else (C.c_int32 * 1)(1)
    check(_L().vila_s2_merge_bwd_bf16(dy.contiguous().data_ptr(), dx.data_ptr(), tile_desc.contiguous().data_ptr(), tile_desc.shape[0], g, Cc,
                                      n_scales, sp, _stream()), "s2_merge_bwd")
    return dx


# ---- LoRA: the three skinny products of a rank-r adapter (vila_amd/csrc/lora.hip) -------------------------------------------------------------
def _lora_ws(n_bytes: int, device) -> Optional[torch.Tensor]:
    return torch.empty((n_bytes,), device=device, dtype=torch.uint8) if n_bytes else None


def lora_down(x: torch.Tensor, a: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, R] = scale * x[M, K] @ a[R, K]^T.  `out` may be a column slice of a wider buffer (the q|k|v stack of the backward)."""
    _need(x, name="x"); _need(a, name="a")
    assert x.dim() == 2 and a.dim() == 2 and x.stride(1) == 1 and a.stride(1) == 1
    if x.shape[1] != a.shape[1]:
        raise ValueError(f"lora_down: contraction widths differ ({x.shape[1]} vs {a.shape[1]})")
    M, K = x.shape
    R = a.shape[0]
    if out is None:
        out = torch.empty((M, R), device=x.device, dtype=torch.bfloat16)
    assert out.shape == (M, R) and out.stride(1) == 1 and out.dtype == torch.bfloat16
    n = int(_L().vila_lora_down_workspace_bytes(M, K, R))
    ws = _lora_ws(n, x.device)
    check(_L().vila_lora_down_bf16(x.data_ptr(), x.stride(0), a.data_ptr(), a.stride(0), out.data_ptr(), out.stride(0), M, K, R, float(scale), _p(ws), n,
                                   _stream()), "lora_down")
    return out


def lora_up(t: torch.Tensor, bt: torch.Tensor, scale: float = 1.0, res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, N] = res + scale * t[M, R] @ bt[R, N].  `t`, `res` and `out` may be column slices; `out` is write-only and `res` aliases nothing."""
    _need(t, name="t"); _need(bt, name="bt")
    assert t.dim() == 2 and bt.dim() == 2 and t.stride(1) == 1 and bt.stride(1) == 1
    if t.shape[1] != bt.shape[0]:
        raise ValueError(f"lora_up: contraction widths differ ({t.shape[1]} vs {bt.shape[0]})")
    M, R = t.shape
    N = bt.shape[1]
    if out is None:
        out = torch.empty((M, N), device=t.device, dtype=torch.bfloat16)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == torch.bfloat16
    if res is not None:
        _need(res, name="res"); assert res.shape == (M, N) and res.stride(1) == 1
    check(_L().vila_lora_up_bf16(t.data_ptr(), t.stride(0), bt.data_ptr(), bt.stride(0), _p(res), res.stride(0) if res is not None else 0, out.data_ptr(),
                                 out.stride(0), M, N, R, float(scale), None, 0, _stream()), "lora_up")
    return out


def lora_wgrad(l: torch.Tensor, x: torch.Tensor, out: torch.Tensor, scale: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """out[R, C] (+)= scale * l[M, R]^T @ x[M, C]: the contraction runs over the rows, both operands are read as they lie."""
    _need(l, name="l"); _need(x, name="x"); _need(out, name="out")
    assert l.dim() == 2 and x.dim() == 2 and l.stride(1) == 1 and x.stride(1) == 1 and out.stride(1) == 1
    if l.shape[0] != x.shape[0]:
        raise ValueError(f"lora_wgrad: row counts differ ({l.shape[0]} vs {x.shape[0]})")
    M, R = l.shape
    C = x.shape[1]
    assert out.shape == (R, C)
    n = int(_L().vila_lora_wgrad_workspace_bytes(M, R, C))
    ws = _lora_ws(n, x.device)
    check(_L().vila_lora_wgrad_bf16(l.data_ptr(), l.stride(0), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), M, R, C, float(scale),
                                    int(accumulate), _p(ws), n, _stream()), "lora_wgrad")
    return out

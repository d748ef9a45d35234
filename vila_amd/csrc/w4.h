// W4A16 decode GEMV (gemv_w4.hip) and prefill GEMM (gemm_w4.hip) arguments.
#pragma once
#include "common.h"

struct GemvW4Args {
    const bf16_t* x; const bf16_t* norm_w; float eps;
    const uint32_t* Wq; const uint32_t* Wsz;       // tile-major packed nibbles / {scale, zero} bf16 pairs (layout: gemv_w4.hip header)
    const bf16_t* bias; const bf16_t* residual; bf16_t* y;
    int N, K, mode;                                // N = outputs. 0 plain, 1 gate/up (2N interleaved rows), 3 fused QKV + RoPE + KV append,
                                                   // 4 plain with x = the merge of the decode attention's per-slice partials (o_proj; hd = 128)
    bf16_t* q_out; bf16_t* kcache; bf16_t* vcache; const int32_t* pos_ptr; const float* rope_cs; int nq, nkv, hd, max_ctx;
    const float* part_o; const float* part_ml; int n_splits, split_keys;     // mode 4: [n_splits][K] un-normalised partial O, [n_splits][K/128][2] (m, l)
};
int launch_gemv_w4(const GemvW4Args& a, hipStream_t s);

// Y[M][N] = X[M][K] . W^T on the same packed buffer; mode 0 plain (+bias)(+residual), 1 gate/up (2N interleaved rows -> silu(g) * u),
// 2 qkv (first n_rope_heads heads of width hd RoPE-interleaved -> written in natural column order, + bias).  Row strides: X K, Y and residual N.
struct GemmW4Args {
    const bf16_t* x; const uint32_t* Wq; const uint32_t* Wsz;
    const bf16_t* bias; const bf16_t* residual; bf16_t* y;
    int M, N, K, mode;
    int n_rope_heads, hd;
};
size_t gemm_w4_workspace_bytes(int M, int N, int K, int mode);     // fp32 K-slice slabs of an under-filled grid (0: none)
int launch_gemm_w4(const GemmW4Args& a, void* ws, size_t ws_bytes, hipStream_t s);

// Y[m][N] = X[m][K] . W^T for 1 <= n <= 16 activation rows (gemv_w4_batch.hip), the batched decode's projections on the same packed
// buffer.  mode 0 plain (+bias)(+residual, y may alias it), 1 gate/up (2N interleaved rows -> silu(g) * u), 2 q|k|v + bias + RoPE at each
// row's position + K/V append into row m's cache slot (N = (nq + 2 nkv) hd, q/k heads RoPE-interleaved; rope_cs [n][hd] = cos | sin).
struct GemvW4BatchArgs {
    const bf16_t* x; int64_t ldx;                  // [n][K] activations
    const uint32_t* Wq; const uint32_t* Wsz;
    const bf16_t* bias;                            // [N] optional (modes 0, 2)
    const bf16_t* residual; int64_t ldr;           // [n][N] optional (mode 0)
    bf16_t* y; int64_t ldy;                        // [n][N] (modes 0, 1)
    int n, N, K, mode;
    bf16_t* q_out; int64_t ldq;                    // mode 2: [n][nq*hd]
    bf16_t* kcache; bf16_t* vcache; int64_t slot_stride;     // this layer's [slots][nkv][max_ctx][hd]; row m uses slot m
    const int32_t* pos; const float* rope_cs;      // [n], [n][hd]
    int nq, nkv, hd, max_ctx;
};
int launch_gemv_w4_batch(const GemvW4BatchArgs& a, hipStream_t s);

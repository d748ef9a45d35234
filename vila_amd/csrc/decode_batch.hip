// Batched decode (the serving side of generate — llava/model/llava_arch.py:823-833 with a batch, server.py:171-290
// serving concurrent requests): ONE pass over the weights serves up to 16 sequences.  The batch-1 GEMVs (gemv.hip) become skinny GEMMs on
// the matrix cores: C[batch 16][n 16] += X[batch][k] . W[n][k] with v_mfma_f32_16x16x32_bf16, A = the activations (rows = sequences, zero
// rows beyond the batch), B = 16 weight rows straight from HBM.  The roofline stays HBM (the weight bytes of a token step are read once
// for the whole batch); what changes is the FMA engine: a VALU dot product costs one lane-op per weight element AND sequence.
//
//   * a block = 8 waves = one work item (16 output rows, or a pair of 16-row tiles: gate + up, the rotate-half partners of RoPE) with the
//     64-wide k-blocks dealt round-robin to the waves (consecutive waves read consecutive 128-B lines of a row); partial sums meet in LDS,
//     wave 0 runs the epilogue while the others already stream the next item (one raw barrier per item, double-buffered exchange area);
//   * weights AND activations reach the matrix core through per-wave LDS-DMA rings in whole 128-B lines (bgemm_dma_kernel's header has the
//     why and the numbers); the RMSNorm in front of qkv / gate-up / lm_head is its own launch (elementwise.hip, HF rounding order);
//   * epilogues mirror gemv.hip's rounding exactly: bias, residual, silu(gate) * up, RoPE with the row's own position + KV-cache append into
//     the row's own cache slot, fp32 logits;
//   * attention: one block per (kv head, 256-key slice, sequence) serving the whole GQA group from one K/V read (bdec_attn_kernel).
// History (round 3, batch 8, NVILA-8B, ms per step on one MI355X): register kernel with operand-shaped loads 5.17 -> software-pipelined
// 5.14 -> row-contiguous loads re-dealt by ds_bpermute 6.30 (rejected) -> LDS-DMA rings 3.74 -> GQA-sliced attention 3.59.
#include "../../include/vila_hip.h"
#include "kernels.h"
#include "gemv_common.h"
#include "attn_common.h"
#include "w4.h"
#include <cstdlib>
#include <cstring>


// BGemmCore: what the kernels of a step without adapters take (their kernarg layout is part of their machine code).  BGemmArgs adds the fp32 addend
// of a step with per-row LoRA adapters (lora_decode.hip); a launch with addend == NULL runs the BGemmCore kernel.
struct BGemmCore {
    const bf16_t* x; int64_t ldx;            // [n][K] activations
    const bf16_t* W; const bf16_t* W2;       // [N][K]; W2: up_proj rows (mode 1)
    const bf16_t* bias;                      // [N] optional
    const bf16_t* residual; int64_t ldr;     // [n][N] optional
    bf16_t* y; int64_t ldy;                  // [n][N] bf16 out
    float* y_f32; int64_t ldf;               // [n][N] fp32 out (logits)
    int n, N, K, mode;                       // mode 0 plain, 1 gate/up, 2 qkv (+bias, RoPE, cache append)
    // mode 2
    bf16_t* q_out; int64_t ldq;              // [n][nq*hd]
    bf16_t* kcache; bf16_t* vcache;          // this layer's [slots][nkv][max_ctx][hd]; row i uses slot i
    int64_t slot_stride;
    const int32_t* pos;                      // [n]
    const float* rope_cs;                    // [n][hd]: cos | sin of each row's position
    int nq, nkv, hd, max_ctx;
};
struct BGemmArgs : BGemmCore {
    const float* addend; int64_t lda;        // [n][N] fp32 (mode 1: [n][2 N], gate | up) added to the fp32 sum in front of the bias and the first rounding
    const int32_t* row_adapter;              // [n] optional: a row with row_adapter[m] < 0 skips the add (NOT + 0.0: a sum of -0.0 keeps its sign)
};

// The finishing step of one work item, run by one wave on the block-reduced sums (C layout of v_mfma_f32_16x16x32: sequence m = lg*4 + r,
// output feature n = r0 + l15).  Rounding mirrors gemv.hip / HF: every tensor rounded to bf16.
// ADD (P = BGemmArgs): row m's addend joins the fp32 sum first, so in front of the bias, of silu (mode 1) and of RoPE and the cache append (mode 2).
template <int MODE, int NT, bool ADD, class P>
__device__ __forceinline__ void bgemm_epilogue(const P& p, int item, const int (&r0)[NT], const f32x4 (&sum)[NT], int lane) {
    const int l15 = lane & 15, lg = lane >> 4;
    const int half = p.hd >> 1, gph = half >> 4;
    (void)half; (void)gph; (void)item;
    // C layout: sequence m = lg*4 + r, output feature n = r0 + l15
    if constexpr (MODE == 1) {
        const int n = r0[0] + l15;
        if (n < p.N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = lg * 4 + r;
                if (m < p.n) {
                    float gs = sum[0][r], us = sum[1][r];
                    if constexpr (ADD) {
                        if (p.row_adapter == nullptr || p.row_adapter[m] >= 0) { gs += p.addend[(int64_t)m * p.lda + n]; us += p.addend[(int64_t)m * p.lda + p.N + n]; }
                    }
                    const float gv = bfround(gs), uv = bfround(us);                          // HF: every tensor rounded to bf16
                    p.y[(int64_t)m * p.ldy + n] = f2bf(bfround(silu_f(gv)) * uv);
                }
            }
        }
    } else if constexpr (MODE == 2) {
        const int head = item / gph, j = item % gph;
        const bool is_v = head >= p.nq + p.nkv, is_q = head < p.nq;
        const int gi = j * 16 + l15;                                                         // index inside the half head
        const int na = r0[0] + l15, nb = r0[1] + l15;
        const float ba = p.bias != nullptr ? bf2f(p.bias[na]) : 0.f, bb = p.bias != nullptr ? bf2f(p.bias[nb]) : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = lg * 4 + r;
            if (m >= p.n) continue;
            float sa = sum[0][r], sb = sum[1][r];
            if constexpr (ADD) {
                if (p.row_adapter == nullptr || p.row_adapter[m] >= 0) { sa += p.addend[(int64_t)m * p.lda + na]; sb += p.addend[(int64_t)m * p.lda + nb]; }
            }
            const float lo = bfround(sa + ba), hi = bfround(sb + bb);
            float oa = lo, ob = hi;
            if (!is_v) {
                const float c = p.rope_cs[m * p.hd + gi], sn = p.rope_cs[m * p.hd + half + gi];
                oa = bfround(bfround(lo * c) + bfround(-hi * sn));
                ob = bfround(bfround(hi * c) + bfround(lo * sn));
            }
            if (is_q) {
                p.q_out[(int64_t)m * p.ldq + na] = f2bf(oa);
                p.q_out[(int64_t)m * p.ldq + nb] = f2bf(ob);
            } else {
                const int ps = p.pos[m];
                if (ps < p.max_ctx) {
                    const int kvh = is_v ? head - p.nq - p.nkv : head - p.nq;
                    bf16_t* dst = (is_v ? p.vcache : p.kcache) + (int64_t)m * p.slot_stride + ((int64_t)kvh * p.max_ctx + ps) * p.hd;
                    dst[gi] = f2bf(oa);
                    dst[half + gi] = f2bf(ob);
                }
            }
        }
    } else {
        const int n = r0[0] + l15;
        if (n < p.N) {
            const float bv = p.bias != nullptr ? bf2f(p.bias[n]) : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = lg * 4 + r;
                if (m >= p.n) continue;
                float v = sum[0][r];
                if constexpr (ADD) {
                    if (p.row_adapter == nullptr || p.row_adapter[m] >= 0) v += p.addend[(int64_t)m * p.lda + n];
                }
                v += bv;
                if (p.y_f32 != nullptr) p.y_f32[(int64_t)m * p.ldf + n] = v;
                if (p.y != nullptr) {
                    if (p.residual != nullptr) v = bfround(v) + bf2f(p.residual[(int64_t)m * p.ldr + n]);
                    p.y[(int64_t)m * p.ldy + n] = f2bf(v);
                }
            }
        }
    }
}

// ---- the weight stream through LDS (the kernel the step uses) ------------------------------------------------------------------------
// The MFMA operand layout (lane = row & 15, 16 B per lane) is the wrong shape to LOAD in: one instruction touches 16 rows x 64 B, every
// 128-B line is fetched by two instructions, and with 8 waves x 16+ loads in flight the second one no longer finds it in the 32-KB vector
// cache (tools/exp/stream_bench.hip: 4.5 TB/s, 5.5 without the streaming hint; the round's first kernel, which loaded that way, reached 3.5-3.9).  Whole lines —
// 8 adjacent lanes x 16 B = one 128-B line, 8 rows per instruction — stream at 6.2 TB/s, but put a row's chunks in 8 different lanes.
// So the lines go through LDS: `global_load_lds` (no VGPRs, lane-linear 1-KB image per instruction) with the XOR swizzle applied to the
// SOURCE chunk (slot s of row r holds chunk s ^ ((r >> 1) & 7)), and ds_read_b128 hands each lane its operand (conflict-free under
// gfx950's b128 lane groups {0-3,12-15,20-27},...: 16 distinct rows per group, 8 of them one k-group further).  The activations take the
// same road (an [XR][128 B] slice per k-block, L2-resident), so the kernel has no staging phase and no K limit; the RMSNorm in front
// becomes its own small launch.  Each wave owns a private ring of NS slots (one slot = one 64-wide k-block: NT x 2 KB of weights +
// XR x 128 B of activations), refilled as soon as a slot is consumed, counted s_waitcnt vmcnt; the only block-wide event is the
// exchange of the 8 partial sums at an item's end (raw s_barrier: __syncthreads() would drain the rings).
// Measured and rejected: carrying the RMSNorm inside this kernel (raw slices in the rings, w * bf16(x * rstd) applied to every A fragment
// between its ds_read and its MFMA, rstd per block in a prologue).  The fragment is re-normalised for every work item and wave, and with
// software rounding that is ~240 VALU ops per k-block: gate/up 46.8 -> 67 us, lm_head 180 -> 414 us; with v_cvt_pk_bf16_f32 the step is
// 3.64 ms against 3.60 with the two 5-us norm launches per layer — not worth a second code path.
template <int MODE, int XR, bool ADD = false>
__global__ __launch_bounds__(512) void bgemm_dma_kernel(std::conditional_t<ADD, BGemmArgs, BGemmCore> p, int n_items) {
    constexpr int NT = (MODE == 1 || MODE == 2) ? 2 : 1;
    constexpr int XI = XR / 8;                               // DMA instructions per activation slice
    constexpr int DPS = NT * 2 + XI;                         // DMA instructions per slot
    constexpr int SLOT = DPS * 1024;
    constexpr int RING = 16384;                              // per wave
    constexpr int NS = RING / SLOT;                          // 3 (two tiles, 8 rows) .. 5 (one tile, 8 rows); 2 for two tiles at 16 rows
    static_assert(NS >= 2 && NS <= 5, "ring depth");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int K = p.K, nkb = K >> 6;
    char* ring = smem + wave * RING;
    float* red = (float*)(smem + 8 * RING);                  // [2 parities][8 waves][NT][64 lanes] f32x4
    const int nkw = nkb > wave ? (nkb - wave + 7) >> 3 : 0;  // this wave's k-blocks: wave, wave + 8, ...
    const int half = p.hd >> 1, gph = half >> 4;
    auto tile_rows = [&](int item, int (&r0)[NT]) {
        if constexpr (MODE == 2) {
            const int head = item / gph, j = item % gph;
            r0[0] = head * p.hd + j * 16; r0[1] = r0[0] + half;
        } else if constexpr (MODE == 1) {
            r0[0] = item * 16; r0[1] = item * 16;
        } else {
            r0[0] = item * 16;
        }
    };
    // DMA side: lane = (row8 = lane >> 3, slot = lane & 7) of an 8-row x 128-B piece; the swizzle picks the source chunk
    const int d_row = lane >> 3, d_slot = lane & 7;
    const bf16_t* xsrc[XI];
#pragma unroll
    for (int j = 0; j < XI; ++j) {
        const int m = 8 * j + d_row, mc = m < p.n ? m : p.n - 1;                   // (rows beyond the batch: a copy of the last one, never stored)
        xsrc[j] = p.x + (int64_t)mc * p.ldx + ((d_slot ^ ((m >> 1) & 7)) << 3);
    }
    struct Cur { int item, i; };
    auto issue = [&](Cur c, int slot) {
        const int kb = wave + 8 * c.i;
        int r0[NT];
        tile_rows(c.item, r0);
        char* dst = ring + slot * SLOT;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bf16_t* wbase = (MODE == 1 && t == 1) ? p.W2 : p.W;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int rl = 8 * j + d_row;
                int n = r0[t] + rl; n = n < p.N ? n : p.N - 1;
                const bf16_t* src = wbase + (int64_t)n * K + kb * 64 + ((d_slot ^ ((rl >> 1) & 7)) << 3);
                __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(dst + (t * 2 + j) * 1024), 16, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < XI; ++j)
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(xsrc[j] + kb * 64), (lds_void_t*)(dst + (NT * 2 + j) * 1024), 16, 0, 0);
    };
    auto advance = [&](Cur& c) { if (++c.i >= nkw) { c.i = 0; c.item += gridDim.x; } };
    // read side: lane (n = l15, k-group lg) wants chunk h*4 + lg of row n for the h-th MFMA of the k-block
    const int offB = (l15 >> 3) * 1024 + (l15 & 7) * 128 + ((lg ^ ((l15 >> 1) & 7)) << 4);
    const int mA = l15 & (XR - 1);
    const int offA = NT * 2048 + (mA >> 3) * 1024 + (mA & 7) * 128 + ((lg ^ ((mA >> 1) & 7)) << 4);

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    Cur ci{(int)blockIdx.x, 0};
    int in_flight = 0, islot = 0, cslot = 0, parity = 0;
    if (nkw > 0) {
#pragma unroll 1
        for (int k = 0; k < NS - 1 && ci.item < n_items; ++k) {
            issue(ci, islot); advance(ci); ++in_flight; if (++islot == NS) islot = 0;
        }
    }
#pragma unroll 1
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
#pragma unroll 1
        for (int i = 0; i < nkw; ++i) {
            if (ci.item < n_items) { issue(ci, islot); advance(ci); ++in_flight; if (++islot == NS) islot = 0; }
            wait_tiles_ahead<DPS, NS - 1>(in_flight - 1);
            --in_flight;
            const char* sp = ring + cslot * SLOT;
            if (++cslot == NS) cslot = 0;
            const u32x4 xa = *(const u32x4*)(sp + offA), xb = *(const u32x4*)(sp + (offA ^ 64));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const u32x4 wa = *(const u32x4*)(sp + t * 2048 + offB), wb = *(const u32x4*)(sp + t * 2048 + (offB ^ 64));
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xa), __builtin_bit_cast(bf16x8, wa), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xb), __builtin_bit_cast(bf16x8, wb), acc[t], 0, 0, 0);
            }
        }
        // ---- the 8 partial sums meet in LDS; wave 0 finishes the item while the others stream the next one ----
        float* rp = red + (size_t)parity * 8 * NT * 256;
        parity ^= 1;
#pragma unroll
        for (int t = 0; t < NT; ++t) { *(f32x4*)(rp + ((wave * NT + t) * 64 + lane) * 4) = acc[t]; acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wave == 0) {
            int r0[NT];
            tile_rows(item, r0);
            f32x4 sum[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                sum[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    const f32x4 a = *(const f32x4*)(rp + ((w * NT + t) * 64 + lane) * 4);
                    sum[t][0] += a[0]; sum[t][1] += a[1]; sum[t][2] += a[2]; sum[t][3] += a[3];
                }
            }
            bgemm_epilogue<MODE, NT, ADD>(p, item, r0, sum, lane);
        }
    }
}
template <int MODE, int XR, bool ADD = false>
static int launch_bgemm_dma_t(const std::conditional_t<ADD, BGemmArgs, BGemmCore>& a, int n_items, hipStream_t s) {
    constexpr int NT = (MODE == 1 || MODE == 2) ? 2 : 1;
    const size_t lds = (size_t)8 * 16384 + (size_t)2 * 8 * NT * 256 * 4;
    static bool attr = false;
    if (!attr) {
        VILA_HIP(hipFuncSetAttribute((const void*)bgemm_dma_kernel<MODE, XR, ADD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    const int grid = n_items < 256 ? n_items : 256;
    hipLaunchKernelGGL((bgemm_dma_kernel<MODE, XR, ADD>), dim3(grid), dim3(512), lds, s, a, n_items);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ADD: the kernels with the addend in the epilogue (a step with adapters); otherwise the BGemmCore kernels every other step launches
template <bool ADD>
static int launch_bgemm_t(const BGemmArgs& a, hipStream_t s) {
    const bool x8 = a.n <= 8;
    if (a.mode == 1) {
        VILA_REQUIRE(a.W2 != nullptr && a.y != nullptr, "batched decode GEMM: gate/up needs W2 and a bf16 output");
        return x8 ? launch_bgemm_dma_t<1, 8, ADD>(a, cdiv(a.N, 16), s) : launch_bgemm_dma_t<1, 16, ADD>(a, cdiv(a.N, 16), s);
    }
    if (a.mode == 2) {
        VILA_REQUIRE(a.hd % 32 == 0 && a.N == (a.nq + 2 * a.nkv) * a.hd && a.q_out && a.kcache && a.vcache && a.pos && a.rope_cs,
                     "batched decode GEMM: qkv mode needs head_dim %% 32 == 0 and its outputs");
        const int items = (a.nq + 2 * a.nkv) * (a.hd / 32);
        return x8 ? launch_bgemm_dma_t<2, 8, ADD>(a, items, s) : launch_bgemm_dma_t<2, 16, ADD>(a, items, s);
    }
    return x8 ? launch_bgemm_dma_t<0, 8, ADD>(a, cdiv(a.N, 16), s) : launch_bgemm_dma_t<0, 16, ADD>(a, cdiv(a.N, 16), s);
}
static int launch_bgemm(const BGemmArgs& a, hipStream_t s) {
    VILA_REQUIRE(a.n >= 1 && a.n <= 16, "batched decode: 1..16 sequences (got %d)", a.n);
    VILA_REQUIRE(a.K % 64 == 0 && a.K > 0 && a.N > 0, "batched decode GEMM: K (%d) must be a positive multiple of 64", a.K);
    VILA_REQUIRE((uintptr_t)a.W % 16 == 0 && (uintptr_t)a.x % 16 == 0 && a.ldx % 8 == 0, "batched decode GEMM: operand alignment");
    if (a.addend == nullptr) return launch_bgemm_t<false>(a, s);
    VILA_REQUIRE(a.lda >= (a.mode == 1 ? 2 : 1) * (int64_t)a.N, "batched decode GEMM: the addend's row stride (%lld) is shorter than its row", (long long)a.lda);
    return launch_bgemm_t<true>(a, s);
}

// ---- per-row prologue / pick / advance -------------------------------------------------------------------------------------------
// x[row] = embed[token[row]]; rope table of the row's position: cs[row][0:hd/2] = cos, [hd/2:hd] = sin, rounded to bf16 like HF
__global__ void bdec_prologue_kernel(const bf16_t* __restrict__ table, const int64_t* __restrict__ tok, bf16_t* __restrict__ out, int H, int64_t vocab,
                                     const int32_t* __restrict__ pos, float* __restrict__ rope_cs, int hd, float theta) {
    const int row = blockIdx.y;
    int64_t id = tok[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < (H >> 3); c += gridDim.x * blockDim.x)
        *(u32x4*)(out + (int64_t)row * H + c * 8) = *(const u32x4*)(table + id * H + c * 8);
    if (blockIdx.x == 0 && (int)threadIdx.x < (hd >> 1)) {
        const int d = threadIdx.x;
        const float inv = 1.0f / powf(theta, (float)(2 * d) / (float)hd);
        const float ang = (float)pos[row] * inv;
        rope_cs[row * hd + d] = bfround(cosf(ang));
        rope_cs[row * hd + (hd >> 1) + d] = bfround(sinf(ang));
    }
}
// greedy pick per row (first index of the maximum, like argmax_stage1/2) and the state advance.  Two launches: PICK_SLICES blocks per row each
// scan a slice of the vocabulary (one block per row took 72 us for 8 x 152064 logits on 8 CUs), then one small block per row merges and advances.
#define PICK_SLICES 32
__global__ __launch_bounds__(256) void bdec_pick1_kernel(const float* __restrict__ logits, int V, float* __restrict__ pv, int* __restrict__ pi) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int row = blockIdx.y, sl = blockIdx.x;
    const int per = (V + PICK_SLICES - 1) / PICK_SLICES, lo = sl * per, hi = lo + per < V ? lo + per : V;
    const float* lr = logits + (int64_t)row * V;
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int i = lo + threadIdx.x; i < hi; i += 256) { const float v = lr[i]; if (v > best || (v == best && i < bi)) { best = v; bi = i; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, 64); const int i2 = __shfl_xor(bi, o, 64);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        pv[row * PICK_SLICES + sl] = best; pi[row * PICK_SLICES + sl] = bi;
    }
}
__global__ __launch_bounds__(64) void bdec_pick2_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int64_t* __restrict__ token,
                                                        int32_t* __restrict__ pos, int64_t* __restrict__ out_ids, int32_t* __restrict__ n_out, int max_out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    float best = lane < PICK_SLICES ? pv[row * PICK_SLICES + lane] : -INFINITY;
    int bi = lane < PICK_SLICES ? pi[row * PICK_SLICES + lane] : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, 64); const int i2 = __shfl_xor(bi, o, 64);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if (lane == 0) {
        token[row] = (int64_t)bi;
        const int n = n_out[row];
        if (n < max_out) out_ids[(int64_t)row * max_out + n] = (int64_t)bi;
        n_out[row] = n + 1;
        pos[row] = pos[row] + 1;
    }
}

// ---- what the batched step and the verify step share: the workspace layout and the forward of n rows ------------------------------------
struct BStepBufs {
    bf16_t *x, *x2, *xn, *q, *ao, *act; float* rope_cs; float *part_o, *part_ml; float* pick_v; int* pick_i;
    int32_t* pos_rows;                                       // the verify step's per-row positions
    void* smp_ws; int64_t* draws;                            // the sampled verify step's sampler candidates and its n draws
    float *pfx_o, *pfx_ml;                                   // the prefix step's prefix-phase partials
};
// The size functions below bound this layout: bdec_step_common_bytes counts every take() but the attention partials and pos_rows at its aligned size,
// and each step adds its own term for those.  The partials are two separately aligned arrays (part_o, part_ml) where the batched step's term is one
// aligned sum plus 256: align(a) + align(b) <= align(a + b) + 256, since rounding two parts up can overshoot rounding their sum by less than one
// more unit.  The verify step's term is bverify_attn_workspace_bytes, the two aligned arrays themselves.  The 4096 on top is slack.
// draws: the sampled verify step's two arrays behind everything else, each counted at its aligned size by bverify_sample_workspace_bytes.
// psl > 0: the prefix step's second set of partials behind everything else, bverify_attn_workspace_bytes in bdecode_prefix_workspace_bytes.
static bool bdec_carve(void* workspace, size_t workspace_bytes, int n, int H, int F, int QS, int hd, int nq, int nsl, bool pos_rows, bool draws, BStepBufs* b,
                       int psl = 0) {
    char* wp = (char*)workspace; size_t off = 0;
    auto take = [&](size_t bytes) { off = align_up(off, 256); void* r = wp + off; off += bytes; return r; };
    b->x = (bf16_t*)take((size_t)n * H * 2);
    b->x2 = (bf16_t*)take((size_t)n * H * 2);
    b->xn = (bf16_t*)take((size_t)n * H * 2);                // the normalised activations in front of qkv / gate-up / lm_head
    b->q = (bf16_t*)take((size_t)n * QS * 2);
    b->ao = (bf16_t*)take((size_t)n * QS * 2);
    b->act = (bf16_t*)take((size_t)n * F * 2);
    b->rope_cs = (float*)take((size_t)n * hd * 4);
    b->part_o = (float*)take((size_t)n * nq * nsl * hd * 4);
    b->part_ml = (float*)take((size_t)n * nq * nsl * 2 * 4);
    b->pick_v = (float*)take((size_t)n * PICK_SLICES * 4);
    b->pick_i = (int*)take((size_t)n * PICK_SLICES * 4);
    b->pos_rows = pos_rows ? (int32_t*)take((size_t)n * 4) : nullptr;
    b->smp_ws = draws ? take(sample_batch_workspace_bytes(n)) : nullptr;
    b->draws = draws ? (int64_t*)take((size_t)n * 8) : nullptr;
    b->pfx_o = psl > 0 ? (float*)take((size_t)n * nq * psl * hd * 4) : nullptr;
    b->pfx_ml = psl > 0 ? (float*)take((size_t)n * nq * psl * 2 * 4) : nullptr;
    return off <= workspace_bytes;
}
// embed + rope table, the layers, lm_head -> logits [n][vocab].  Row i appends its K/V at position pos[i] of kcache/vcache + i * slot_stride (+ the
// layer); attn(q, kc, vc, ao) enqueues the layer's attention on that layer's cache.
template <class Attn>
static int bdec_forward(const BDecodeArgs& m, const BLayer* layers, const BLayerW4* qlayers, bf16_t* kcache, bf16_t* vcache, int64_t per_layer, int64_t slot_stride,
                        int max_ctx, int n, const int32_t* pos, const int64_t* token, float* logits, const BStepBufs& b, hipStream_t s, Attn&& attn,
                        const BLora* lora = nullptr) {
    const int H = m.hidden, F = m.inter, hd = m.head_dim, QS = m.q_heads * hd, KS = m.kv_heads * hd;
    bf16_t* x = b.x; bf16_t* x2 = b.x2; bf16_t* xn = b.xn; bf16_t* q = b.q; bf16_t* ao = b.ao; bf16_t* act = b.act; float* rope_cs = b.rope_cs;
    auto normed = [&](BGemmArgs& g, const bf16_t* src, const void* w) -> int {
        VILA_TRY(launch_rmsnorm(src, (const bf16_t*)w, xn, n, H, m.rms_eps, s));
        g.x = xn;
        return 0;
    };
    // the four projections: bf16 skinny GEMMs, or with int4 layers the W4A16 batched GEMV on the same operands and epilogue
    auto proj = [&](const BGemmArgs& g, const void* wq, const void* wsz) -> int {
        if (qlayers == nullptr) return launch_bgemm(g, s);
        GemvW4BatchArgs a{};
        a.x = g.x; a.ldx = g.ldx; a.Wq = (const uint32_t*)wq; a.Wsz = (const uint32_t*)wsz; a.bias = g.bias; a.residual = g.residual; a.ldr = g.ldr;
        a.y = g.y; a.ldy = g.ldy; a.n = g.n; a.N = g.N; a.K = g.K; a.mode = g.mode;
        a.q_out = g.q_out; a.ldq = g.ldq; a.kcache = g.kcache; a.vcache = g.vcache; a.slot_stride = g.slot_stride; a.pos = g.pos; a.rope_cs = g.rope_cs;
        a.nq = g.nq; a.nkv = g.nkv; a.hd = g.hd; a.max_ctx = g.max_ctx;
        return launch_gemv_w4_batch(a, s);
    };
    // lora != nullptr (bf16 layers only): in front of a projection, shrink and expand of the rows' adapters on the projection's own input (lora_decode.hip)
    // into lora->D [n][Ntot], which the GEMM's epilogue adds to its fp32 sum; columns [0, c1) | [c1, c2) | [c2, Ntot) are the members of the stack
    auto adapt = [&](BGemmArgs& g, const void* A, const void* Bp, int Ntot, int c1, int c2) -> int {
        if (lora == nullptr) return 0;
        const int r = lora->r, Rs = (1 + (c1 < Ntot) + (c2 < Ntot)) * r;
        VILA_TRY(launch_lora_shrink(g.x, g.ldx, n, (const bf16_t*)A, (int64_t)Rs * g.K, lora->scale, lora->row_adapter, lora->capacity, lora->T, Rs, Rs, g.K, s));
        VILA_TRY(launch_lora_expand(lora->T, Rs, n, (const bf16_t*)Bp, (int64_t)r * Ntot, lora->row_adapter, lora->capacity, lora->D, Ntot, Ntot, r, c1, c2, s));
        g.addend = lora->D; g.lda = Ntot; g.row_adapter = lora->row_adapter;
        return 0;
    };
    hipLaunchKernelGGL(bdec_prologue_kernel, dim3(cdiv(H / 8, 256), n), dim3(256), 0, s, (const bf16_t*)m.embed, token, x, H, (int64_t)m.vocab, pos, rope_cs, hd, m.rope_theta);
    VILA_LAUNCH_CHECK();
    bf16_t* cur = x; bf16_t* nxt = x2;
    for (int l = 0; l < m.n_layers; ++l) {
        const BLayer& L = layers[l];
        const BLayerW4 Q = qlayers != nullptr ? qlayers[l] : BLayerW4{};
        const BLoraLayer A = lora != nullptr ? lora->layers[l] : BLoraLayer{};
        bf16_t* kc = kcache + l * per_layer; bf16_t* vc = vcache + l * per_layer;
        BGemmArgs qa{};
        VILA_TRY(normed(qa, cur, L.ln1_w));
        qa.ldx = H; qa.W = (const bf16_t*)L.wqkv; qa.bias = (const bf16_t*)L.bqkv;
        qa.n = n; qa.N = QS + 2 * KS; qa.K = H; qa.mode = 2; qa.q_out = q; qa.ldq = QS; qa.kcache = kc; qa.vcache = vc; qa.slot_stride = slot_stride;
        qa.pos = pos; qa.rope_cs = rope_cs; qa.nq = m.q_heads; qa.nkv = m.kv_heads; qa.hd = hd; qa.max_ctx = max_ctx;
        VILA_TRY(adapt(qa, A.a_qkv, A.b_qkv, QS + 2 * KS, QS, QS + KS));
        VILA_TRY(proj(qa, Q.qkv_q, Q.qkv_sz));
        VILA_TRY(attn(q, kc, vc, ao));
        BGemmArgs o{};
        o.x = ao; o.ldx = QS; o.W = (const bf16_t*)L.wo; o.residual = cur; o.ldr = H; o.y = nxt; o.ldy = H; o.n = n; o.N = H; o.K = QS; o.mode = 0;
        VILA_TRY(adapt(o, A.a_o, A.b_o, H, H, H));
        VILA_TRY(proj(o, Q.o_q, Q.o_sz));
        BGemmArgs gu{};
        VILA_TRY(normed(gu, nxt, L.ln2_w));
        gu.ldx = H; gu.W = (const bf16_t*)L.w_gate; gu.W2 = (const bf16_t*)L.w_up;
        gu.y = act; gu.ldy = F; gu.n = n; gu.N = F; gu.K = H; gu.mode = 1;
        VILA_TRY(adapt(gu, A.a_gateup, A.b_gateup, 2 * F, F, 2 * F));
        VILA_TRY(proj(gu, Q.gateup_q, Q.gateup_sz));
        BGemmArgs dn{};
        dn.x = act; dn.ldx = F; dn.W = (const bf16_t*)L.w_down; dn.residual = nxt; dn.ldr = H; dn.y = cur; dn.ldy = H; dn.n = n; dn.N = H; dn.K = F; dn.mode = 0;
        VILA_TRY(adapt(dn, A.a_down, A.b_down, H, H, H));
        VILA_TRY(proj(dn, Q.down_q, Q.down_sz));
    }
    BGemmArgs lm{};
    VILA_TRY(normed(lm, cur, m.norm_w));
    lm.ldx = H; lm.W = (const bf16_t*)m.lm_head; lm.y_f32 = logits; lm.ldf = m.vocab;
    lm.n = n; lm.N = m.vocab; lm.K = H; lm.mode = 0;
    VILA_TRY(launch_bgemm(lm, s));
    return 0;
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// what both steps carve whatever their attention: the six activation buffers, the RoPE table, the two pick-partials arrays, and the slack
static size_t bdec_step_common_bytes(int H, int F, int QS, int hd, int n) {
    return 3 * align_up((size_t)n * H * 2, 256) + 2 * align_up((size_t)n * QS * 2, 256) + align_up((size_t)n * F * 2, 256) +
           align_up((size_t)n * hd * 4, 256) + 2 * align_up((size_t)n * PICK_SLICES * 4, 256) + 4096;
}
size_t bdecode_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx) {
    return bdec_step_common_bytes(H, F, QS, hd, n) + align_up((size_t)n * (QS / hd) * bdec_ws_slices(max_ctx) * (hd + 2) * 4, 256) + 256;   // + attention slice partials
}
// the prefix step: the plain step's layout and, behind it, the prefix phase's partials (two aligned arrays; + 256 for the take() in front of them)
size_t bdecode_prefix_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx) {
    return align_up(bdecode_workspace_bytes(H, F, QS, hd, n, max_ctx), 256) + bverify_attn_workspace_bytes(n, QS / hd, max_ctx) + 256;
}

int bdecode_step(const BDecodeArgs& m, const BLayer* layers, bf16_t* kcache, bf16_t* vcache, int max_ctx, int n_slots, int n, int32_t* pos, int64_t* token,
                 int64_t* out_ids, int32_t* n_out, int max_out, float* logits, void* workspace, size_t workspace_bytes, hipStream_t s,
                 const BLayerW4* qlayers, const BatchSampling* sampling, void* sampling_ws, const BPrefix* prefix, const Penalties* pen, float* pen_out,
                 const Constraints* con, bool any_k, const BLora* lora) {
    static_assert(PEN_PICK_SLICES == PICK_SLICES, "the penalty launch writes the pairs bdec_pick2_kernel merges");
    const int H = m.hidden, F = m.inter, hd = m.head_dim, QS = m.q_heads * hd;
    VILA_REQUIRE((pen == nullptr && con == nullptr) || pen_out != nullptr, "batched decode: the penalised / constrained pick needs its scratch rows");
    if (prefix != nullptr) {
        VILA_REQUIRE(prefix->shared_len != nullptr && prefix->uses != nullptr, "batched decode (shared prefix): NULL argument");
        VILA_REQUIRE(n >= 1 && n < n_slots && prefix->prefix_slot >= n && prefix->prefix_slot < n_slots,
                     "batched decode (shared prefix): the prefix slot (%d) is a slot of the cache (%d slots) behind the %d rows' own", prefix->prefix_slot, n_slots, n);
        VILA_REQUIRE(hd == 128 && m.q_heads % m.kv_heads == 0 && bdec_group_ok(m.q_heads / m.kv_heads),
                     "batched decode (shared prefix): head_dim 128 and a GQA group of 1, 2, 4, 7 or 8 query heads per kv head (got %d / %d)", m.q_heads, m.kv_heads);
        VILA_REQUIRE(max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX && workspace_bytes >= bdecode_prefix_workspace_bytes(H, F, QS, hd, n, max_ctx),
                     "batched decode (shared prefix): the step needs the workspace of vila_llm_decode_batch_prefix*_workspace_bytes (%d positions)", max_ctx);
    }
    VILA_REQUIRE(n >= 1 && n <= 16 && n <= n_slots, "batched decode: %d sequences need 1..16 KV-cache slots (cache has %d)", n, n_slots);
    VILA_REQUIRE(QS == H, "batched decode: q_heads*head_dim (%d) must equal hidden (%d)", QS, H);
    VILA_REQUIRE(hd == 128 && max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX, "batched decode: head_dim 128 and caches up to %d positions (got %d, %d)", BDEC_MAX_CTX, hd,
                 max_ctx);
    const BAttnForm form = bdec_attn_form(max_ctx);
    VILA_REQUIRE(!form.walk || (m.q_heads % m.kv_heads == 0 && bdec_group_ok(m.q_heads / m.kv_heads)),
                 "batched decode: caches beyond 2048 positions need a GQA group of 1, 2, 4, 7 or 8 query heads per kv head (got %d / %d)", m.q_heads, m.kv_heads);
    VILA_REQUIRE(max_ctx <= BDEC_SHORT_CTX || workspace_bytes >= bdecode_workspace_bytes(H, F, QS, hd, n, max_ctx),
                 "batched decode: caches beyond 2048 positions need the workspace of vila_llm_decode_batch*_workspace_bytes_ctx (%d positions)", max_ctx);
    VILA_REQUIRE(qlayers == nullptr || (H % 128 == 0 && F % 128 == 0),
                 "batched W4 decode: hidden (%d) and intermediate (%d) must be multiples of the 128-wide quantisation group", H, F);
    VILA_REQUIRE(workspace_bytes >= bdecode_workspace_bytes(H, F, QS, hd, n, max_ctx), "batched decode: workspace too small");
    VILA_REQUIRE(sampling == nullptr || sampling_ws != nullptr, "batched decode: the sampled pick needs its workspace");
    if (lora != nullptr) {
        VILA_REQUIRE(qlayers == nullptr && prefix == nullptr, "batched decode (adapters): the step with per-row adapters has no int4 and no shared-prefix form");
        VILA_REQUIRE(lora->layers != nullptr && lora->scale != nullptr && lora->row_adapter != nullptr && lora->T != nullptr && lora->D != nullptr,
                     "batched decode (adapters): NULL argument");
        VILA_REQUIRE((lora->r == 16 || lora->r == 32 || lora->r == 48 || lora->r == 64) && lora->capacity >= 1 && lora->capacity <= LORA_MAX_SLOTS && F % 64 == 0,
                     "batched decode (adapters): rank 16, 32, 48 or 64, 1..%d slots, intermediate %% 64 == 0 (got r %d, %d slots)", LORA_MAX_SLOTS, lora->r, lora->capacity);
    }
    VILA_REQUIRE(!any_k || sampling != nullptr, "batched decode: any top_k is an option of the sampled pick");
    BStepBufs b{};
    VILA_REQUIRE(bdec_carve(workspace, workspace_bytes, n, H, F, QS, hd, m.q_heads, form.nsl, false, false, &b, prefix != nullptr ? bverify_attn_slices(max_ctx) : 0),
                 "batched decode: workspace layout");
    const int64_t per_layer = (int64_t)n_slots * m.kv_heads * max_ctx * hd, slot_stride = (int64_t)m.kv_heads * max_ctx * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    auto attn = [&](const bf16_t* q, bf16_t* kc, bf16_t* vc, bf16_t* ao) -> int {
        if (prefix != nullptr)
            return bprefix_attn_launch(q, QS, kc, vc, slot_stride, prefix->prefix_slot, prefix->shared_len, prefix->uses, pos, ao, QS, n, m.q_heads, m.kv_heads,
                                       max_ctx, scale, b.part_o, b.part_ml, b.pfx_o, b.pfx_ml, s);
        const int rc = bdecode_attn_launch(form, q, QS, kc, vc, slot_stride, pos, ao, QS, n, m.q_heads, m.kv_heads, max_ctx, scale, b.part_o, b.part_ml, s);
        if (rc < 0) return rc;
        if (rc == 1) {                                                                       // group size without an instantiation: one block per query head
            AttnDecodeArgs ad{};
            ad.q = q; ad.kcache = kc; ad.vcache = vc; ad.o = ao; ad.pos_ptr = pos; ad.nq = m.q_heads; ad.nkv = m.kv_heads; ad.hd = hd; ad.max_ctx = max_ctx;
            ad.n_splits = cdiv(max_ctx, 64); ad.scale = scale;
            VILA_TRY(launch_attn_decode_rows(ad, n, QS, QS, slot_stride, s));
        }
        return 0;
    };
    VILA_TRY(bdec_forward(m, layers, qlayers, kcache, vcache, per_layer, slot_stride, max_ctx, n, pos, token, logits, b, s, attn, lora));
    float* pick_v = b.pick_v; int* pick_i = b.pick_i;
    // the pick: per-row sampling (sample.hip; greedy rows included, position = the draw's counter, read before it advances) or the greedy pair
    // penalised: one launch bumps each row's count of the token it consumed (token[] still holds it), writes the processed rows to pen_out and, for the
    // greedy pick, the pairs bdec_pick1_kernel would have written; the sampler reads pen_out in place of the logits, which stay raw
    const float* pick_src = logits;
    if (pen != nullptr) {
        VILA_TRY(launch_penalize(logits, m.vocab, n, m.vocab, *pen, token, pen_out, m.vocab, PICK_SLICES, sampling != nullptr ? nullptr : pick_v,
                                 sampling != nullptr ? nullptr : pick_i, s));
        pick_src = pen_out;
    }
    // constrained: behind the penalties (in place on pen_out then), the rows' automata advance by the consumed token and mask the row; the pairs of
    // the greedy pick are this launch's, which replace the penalty launch's
    if (con != nullptr) {
        VILA_TRY(launch_constrain(pick_src, m.vocab, n, m.vocab, *con, token, pen_out, m.vocab, PICK_SLICES, sampling != nullptr ? nullptr : pick_v,
                                  sampling != nullptr ? nullptr : pick_i, s));
        pick_src = pen_out;
    }
    if (sampling != nullptr)
        return launch_sample_batch(pick_src, m.vocab, n, m.vocab, *sampling, 1, pos, token, sampling_ws, nullptr, pos, out_ids, n_out, max_out, s, any_k);
    if (pen == nullptr && con == nullptr) {
        hipLaunchKernelGGL(bdec_pick1_kernel, dim3(PICK_SLICES, n), dim3(256), 0, s, logits, m.vocab, pick_v, pick_i);
        VILA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bdec_pick2_kernel, dim3(n), dim3(64), 0, s, pick_v, pick_i, token, pos, out_ids, n_out, max_out);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ---- the verify step: speculative decoding with lookup drafts, greedy or sampled ------------------------------------------------------------
// One sequence, one slot.  token[0] is the last chosen token (not yet in the cache), token[1..n_draft] are guesses at what follows it.  The n rows run
// as consecutive positions pos .. pos + n - 1 of the slot (slot_stride 0: row i's K/V lands at position pos + i), so row i's logits are the model's
// answer to "what follows token[0..i]", and the guesses are accepted as far as the answers reproduce them.  Every accepted token is the greedy
// token of its position, computed by the same arithmetic whatever the drafts were (attn_decode.hip, the shared form's invariance), so the ids are
// those of drafting nothing.  Rows beyond 1 + n_draft are padding: they compute (the graph is fixed) and write K/V past the accepted length,
// which a later step overwrites before any column may see it.
// The sampled form changes only where a[i] comes from: row i DRAWS it with the batched sampler (sample.hip) from the request's parameters and seed
// and the counter pos + i.  The solo sampled step draws the token behind position p with counter p from the same logits bits, so a[i] is again the
// token the session would have chosen one by one, and "the draft equals the draw" keeps the ids those of drafting nothing.
// The draft: HF PromptLookupCandidateGenerator on hist[0 : n_hist] (the ids so far, token[0] last) — for ngram = min(max_ngram, n_hist - 1) .. 1 the
// EARLIEST window equal to the last ngram ids that has something behind it, and up to n - 1 ids from there; or, in candidate mode (cand != NULL and
// *n_cand >= 0), cand[n_out + j]: the candidate's guess for the very output index the row decides, so a rejection re-aligns by itself.
// Also writes the rows' positions for the forward.  One block.
__global__ __launch_bounds__(1024) void bver_draft_kernel(const int64_t* __restrict__ hist, const int32_t* __restrict__ n_hist_p, int max_ngram,
                                                          const int64_t* __restrict__ cand, const int32_t* __restrict__ n_cand_p,
                                                          const int32_t* __restrict__ n_out_p, int n, int64_t* __restrict__ token, int32_t* __restrict__ n_draft,
                                                          const int32_t* __restrict__ pos, int32_t* __restrict__ pos_rows) {
    __shared__ int best;
    const int tid = threadIdx.x;
    if (pos_rows != nullptr && tid < n) pos_rows[tid] = *pos + tid;
    const int64_t pad = token[0];
    int nd = 0, src = 0;
    const int64_t* from = hist;
    const int nc = (cand != nullptr && n_cand_p != nullptr) ? *n_cand_p : -1;
    if (nc >= 0) {
        const int o = n_out_p != nullptr ? *n_out_p : 0;
        nd = nc - o < n - 1 ? nc - o : n - 1;
        nd = nd < 0 ? 0 : nd;
        src = o; from = cand;
    } else {
        const int nh = *n_hist_p;
        for (int ng = (max_ngram < nh - 1 ? max_ngram : nh - 1); ng >= 1 && nd == 0; --ng) {
            __syncthreads();
            if (tid == 0) best = 0x7fffffff;
            __syncthreads();
            // windows s .. s + ng - 1 with s + ng < nh: the tail itself (s = nh - ng) has nothing behind it
            for (int s0 = tid; s0 + ng < nh; s0 += 1024) {
                bool eq = true;
                for (int j = 0; j < ng && eq; ++j) eq = hist[s0 + j] == hist[nh - ng + j];
                if (eq) { atomicMin(&best, s0); break; }         // a thread's windows ascend: its first match is its earliest
            }
            __syncthreads();
            if (best != 0x7fffffff) { src = best + ng; nd = nh - src < n - 1 ? nh - src : n - 1; }
        }
    }
    // (token[0] was read by every thread before the barrier-free stores below can matter: they touch token[1..] only)
    if (tid >= 1 && tid < n) token[tid] = tid <= nd ? from[src + tid - 1] : pad;
    if (tid == 0) *n_draft = nd;
}
int launch_verify_draft(const int64_t* hist, const int32_t* n_hist, int max_ngram, const int64_t* cand, const int32_t* n_cand, const int32_t* n_out, int n,
                        int64_t* token, int32_t* n_draft, const int32_t* pos, int32_t* pos_rows, hipStream_t s) {
    VILA_REQUIRE(n >= 1 && n <= 16 && token != nullptr && n_draft != nullptr && (cand != nullptr || (hist != nullptr && n_hist != nullptr)) && max_ngram >= 1 &&
                 (pos_rows == nullptr || pos != nullptr), "verify draft: 1..16 rows, a history or a candidate, max_ngram >= 1");
    hipLaunchKernelGGL(bver_draft_kernel, dim3(1), dim3(1024), 0, s, hist, n_hist, max_ngram, cand, n_cand, n_out, n, token, n_draft, pos, pos_rows);
    VILA_LAUNCH_CHECK();
    return 0;
}
// The accept rule, by ONE thread, on the rows' choices a[0..n-1] (greedy picks or draws): m = the longest prefix of drafts with a[j] == token[j + 1];
// a[0..m] go to out_ids and hist, the state moves m + 1 tokens and a[m] is the next token[0].
__device__ __forceinline__ void bver_accept(const int* a, int n, int64_t* __restrict__ token, const int32_t* __restrict__ n_draft, int32_t* __restrict__ pos,
                                            int64_t* __restrict__ out_ids, int32_t* __restrict__ n_out, int max_out, int64_t* __restrict__ hist,
                                            int32_t* __restrict__ n_hist, int hist_cap, int32_t* __restrict__ n_accept) {
    int nd = *n_draft;
    nd = nd < 0 ? 0 : (nd > n - 1 ? n - 1 : nd);
    int m = 0;
    while (m < nd && (int64_t)a[m] == token[m + 1]) ++m;
    const int no = *n_out, nh = hist != nullptr ? *n_hist : 0;
    for (int j = 0; j <= m; ++j) {
        if (no + j < max_out) out_ids[no + j] = (int64_t)a[j];
        if (hist != nullptr && nh + j < hist_cap) hist[nh + j] = (int64_t)a[j];
    }
    *n_out = no + m + 1;
    if (hist != nullptr) *n_hist = nh + m + 1 < hist_cap ? nh + m + 1 : hist_cap;      // (a full history stops growing: later drafts are poorer, never wrong)
    *pos = *pos + m + 1;
    token[0] = (int64_t)a[m];
    *n_accept = m;
}
// The greedy accept: wave i finishes row i's greedy pick a[i] (bdec_pick1_kernel's partials), then the rule.  One block of n waves.
__global__ __launch_bounds__(1024) void bver_accept_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int n, int64_t* __restrict__ token,
                                                           const int32_t* __restrict__ n_draft, int32_t* __restrict__ pos, int64_t* __restrict__ out_ids,
                                                           int32_t* __restrict__ n_out, int max_out, int64_t* __restrict__ hist, int32_t* __restrict__ n_hist,
                                                           int hist_cap, int32_t* __restrict__ n_accept) {
    __shared__ int a[16];
    const int row = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float best = lane < PICK_SLICES ? pv[row * PICK_SLICES + lane] : -INFINITY;
    int bi = lane < PICK_SLICES ? pi[row * PICK_SLICES + lane] : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, 64); const int i2 = __shfl_xor(bi, o, 64);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if (lane == 0) a[row] = bi;
    __syncthreads();
    if (threadIdx.x == 0) bver_accept(a, n, token, n_draft, pos, out_ids, n_out, max_out, hist, n_hist, hist_cap, n_accept);
}
// The sampled accept: a[i] = draws[i], what the batched sampler drew for row i (one wave; n <= 16), then the same rule.
__global__ __launch_bounds__(64) void bver_accept_draws_kernel(const int64_t* __restrict__ draws, int n, int64_t* __restrict__ token,
                                                               const int32_t* __restrict__ n_draft, int32_t* __restrict__ pos, int64_t* __restrict__ out_ids,
                                                               int32_t* __restrict__ n_out, int max_out, int64_t* __restrict__ hist,
                                                               int32_t* __restrict__ n_hist, int hist_cap, int32_t* __restrict__ n_accept) {
    __shared__ int a[16];
    if (threadIdx.x < n && threadIdx.x < 16) a[threadIdx.x] = (int)draws[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) bver_accept(a, n, token, n_draft, pos, out_ids, n_out, max_out, hist, n_hist, hist_cap, n_accept);
}
size_t bverify_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx) {
    return bdec_step_common_bytes(H, F, QS, hd, n) + bverify_attn_workspace_bytes(n, QS / hd, max_ctx) + align_up((size_t)n * 4, 256);   // + partials, pos_rows
}
// the sampled step's workspace: the greedy step's, the batched sampler's candidates for n rows, the n draws
size_t bverify_sample_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx) {
    return align_up(bverify_workspace_bytes(H, F, QS, hd, n, max_ctx), 256) + align_up(sample_batch_workspace_bytes(n), 256) + align_up((size_t)(n > 0 ? n : 0) * 8, 256);
}
// The processed verify step: raw logits -> penalties -> automaton mask -> pick / draw -> accept -> commit (-> records).  Row i is processed as the
// session drafting nothing would process it at the step that consumes token[i]: penalised with the counts behind token[0 .. i] (penalty.hip
// penalize_verify_kernel) and masked from the automaton's state behind them (constrain.hip constrain_chain_kernel), both WITHOUT touching the count
// table or the state; the unchanged pick / sampler / accept read the processed rows, and st.logits stays raw.  Behind the accept one thread commits
// what the step really consumed — token[0 .. m] as they were before the accept overwrote token[0], kept in the workspace — so nothing of a rejected
// draft or a padding row reaches the table or the state.  The records are RAW, one per emitted token, into the ONE sequence's arrays.
// Its workspace: the sampled step's (whatever `sampling`), and behind it the processed rows [n][vocab], the consumed tokens, the chain's states, the
// rows' emitted tokens and record indices, and the logprob launch's workspace.
struct BProcBufs { float* rows; int64_t* consumed; int32_t* states; int64_t* tok_rows; int32_t* rec_rows; void* lp_ws; };
static size_t bverify_proc_head(int H, int F, int QS, int hd, int n, int max_ctx) { return align_up(bverify_sample_workspace_bytes(H, F, QS, hd, n, max_ctx), 256); }
size_t bverify_processed_workspace_bytes(int H, int F, int QS, int hd, int n, int max_ctx, int vocab) {
    const size_t r = (size_t)(n > 0 ? n : 0);
    return bverify_proc_head(H, F, QS, hd, n, max_ctx) + align_up(r * (size_t)(vocab > 0 ? vocab : 0) * 4, 256) + 2 * align_up(r * 8, 256) + 2 * align_up(r * 4, 256) +
           align_up(logprob_workspace_bytes(n), 256) + 256;
}
static bool bverify_proc_carve(void* workspace, size_t workspace_bytes, size_t head, int n, int vocab, BProcBufs* b) {
    char* wp = (char*)workspace; size_t off = head;
    auto take = [&](size_t bytes) { off = align_up(off, 256); void* r = wp + off; off += bytes; return r; };
    b->rows = (float*)take((size_t)n * vocab * 4);
    b->consumed = (int64_t*)take((size_t)n * 8);
    b->states = (int32_t*)take((size_t)n * 4);
    b->tok_rows = (int64_t*)take((size_t)n * 8);
    b->rec_rows = (int32_t*)take((size_t)n * 4);
    b->lp_ws = take(logprob_workspace_bytes(n));
    return off <= workspace_bytes;
}
int bverify_step(const BDecodeArgs& m, const BLayer* layers, bf16_t* kcache, bf16_t* vcache, int max_ctx, int n_slots, const BVerifyState& st, void* workspace,
                 size_t workspace_bytes, hipStream_t s, const BLayerW4* qlayers, const BatchSampling* sampling, bool any_k, const BVerifyProc* proc) {
    const int H = m.hidden, F = m.inter, hd = m.head_dim, QS = m.q_heads * hd, n = st.n;
    const Penalties* pen = proc != nullptr ? proc->pen : nullptr;
    const Constraints* con = proc != nullptr ? proc->con : nullptr;
    const bool lp = proc != nullptr && proc->lp_tok != nullptr;
    BProcBufs pb{};
    if (pen != nullptr || con != nullptr || lp) {
        // everything the plain step checks below holds for the head; the rest is carved here, before any launch
        VILA_REQUIRE(n >= 2 && n <= 16 && m.vocab >= 1, "verify step (processed): 2..16 rows per step, got %d", n);
        VILA_REQUIRE(workspace_bytes >= bverify_processed_workspace_bytes(H, F, QS, hd, n, max_ctx, m.vocab), "verify step (processed): workspace too small");
        VILA_REQUIRE(!lp || ((proc->lp_top == nullptr) == (proc->lp_id == nullptr) && proc->lp_max_rec >= 1), "verify step (processed): the records need both "
                     "top_logprob and top_id, or neither, and max_rec >= 1");
        const size_t head = bverify_proc_head(H, F, QS, hd, n, max_ctx);
        VILA_REQUIRE(bverify_proc_carve(workspace, workspace_bytes, head, n, m.vocab, &pb), "verify step (processed): workspace layout");
        workspace_bytes = head;
    }
    VILA_REQUIRE(n >= 2 && n <= 16, "verify step: 2..16 rows per step (1 committed token + up to 15 drafts), got %d", n);
    VILA_REQUIRE(st.slot >= 0 && st.slot < n_slots, "verify step: slot %d of a cache with %d", st.slot, n_slots);
    VILA_REQUIRE(hd == 128 && QS == H && m.q_heads % m.kv_heads == 0 && bdec_group_ok(m.q_heads / m.kv_heads) && max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX,
                 "verify step: head_dim 128 (got %d), q_heads*head_dim == hidden (%d, %d), a GQA group of 1, 2, 4, 7 or 8 query heads per kv head (got %d / %d) "
                 "and caches up to %d positions (got %d)", hd, QS, H, m.q_heads, m.kv_heads, BDEC_MAX_CTX, max_ctx);
    VILA_REQUIRE(qlayers == nullptr || (H % 128 == 0 && F % 128 == 0),
                 "verify step (W4): hidden (%d) and intermediate (%d) must be multiples of the 128-wide quantisation group", H, F);
    VILA_REQUIRE(st.pos && st.token && st.n_draft && st.out_ids && st.n_out && st.logits && st.n_accept && st.max_out >= 1, "verify step: a NULL state member");
    VILA_REQUIRE(st.cand != nullptr || (st.hist != nullptr && st.n_hist != nullptr && st.hist_cap >= 1), "verify step: neither a history nor a candidate");
    VILA_REQUIRE(st.max_ngram >= 1, "verify step: max_ngram >= 1 (got %d)", st.max_ngram);
    VILA_REQUIRE(workspace_bytes >= (sampling != nullptr ? bverify_sample_workspace_bytes(H, F, QS, hd, n, max_ctx) : bverify_workspace_bytes(H, F, QS, hd, n, max_ctx)),
                 "verify step: workspace too small");
    VILA_REQUIRE(sampling == nullptr || (sampling->temperature && sampling->top_k && sampling->top_p && sampling->seed), "verify step: a NULL sampling array");
    VILA_REQUIRE(!any_k || sampling != nullptr, "verify step: any top_k is an option of the sampled step");
    const int nsl = bverify_attn_slices(max_ctx);
    BStepBufs b{};
    VILA_REQUIRE(bdec_carve(workspace, workspace_bytes, n, H, F, QS, hd, m.q_heads, nsl, true, sampling != nullptr, &b), "verify step: workspace layout");
    VILA_TRY(launch_verify_draft(st.hist, st.n_hist, st.max_ngram, st.cand, st.n_cand, st.n_out, n, st.token, st.n_draft, st.pos, b.pos_rows, s));
    const int64_t slot_elems = (int64_t)m.kv_heads * max_ctx * hd, per_layer = (int64_t)n_slots * slot_elems;
    const float scale = 1.0f / sqrtf((float)hd);
    auto attn = [&](const bf16_t* q, bf16_t* kc, bf16_t* vc, bf16_t* ao) -> int {
        return bverify_attn_launch(q, QS, kc, vc, st.pos, ao, QS, n, m.q_heads, m.kv_heads, max_ctx, scale, b.part_o, b.part_ml, s);
    };
    VILA_TRY(bdec_forward(m, layers, qlayers, kcache + st.slot * slot_elems, vcache + st.slot * slot_elems, per_layer, 0, max_ctx, n, b.pos_rows, st.token,
                          st.logits, b, s, attn));
    // the processing chain in front of the pick / draw (none of it without pen and con: the launch list is then the plain step's).  The greedy pairs
    // are those of the last processing launch, which bver_accept_kernel merges as it merges bdec_pick1_kernel's
    const float* pick_src = st.logits;
    const bool greedy = sampling == nullptr;
    if (pen != nullptr || con != nullptr)
        VILA_TRY(launch_verify_chain(con, st.token, n, m.vocab, pb.states, pb.consumed, s));     // the chain's states, and token[] before the accept overwrites it
    if (pen != nullptr) {
        VILA_TRY(launch_penalize_verify(pick_src, m.vocab, n, m.vocab, *pen, st.token, pb.rows, m.vocab, PICK_SLICES, greedy && con == nullptr ? b.pick_v : nullptr,
                                        greedy && con == nullptr ? b.pick_i : nullptr, s));
        pick_src = pb.rows;
    }
    if (con != nullptr) {
        VILA_TRY(launch_constrain_rows(pick_src, m.vocab, n, m.vocab, *con, pb.states, pb.rows, m.vocab, PICK_SLICES, greedy ? b.pick_v : nullptr,
                                       greedy ? b.pick_i : nullptr, s));
        pick_src = pb.rows;
    }
    if (sampling != nullptr) {
        // row i draws a[i] with counter pos_rows[i] = pos + i (written by the draft kernel; pos moves only in the accept below) from entry 0 of the
        // one-entry parameter arrays (stride 0), into the workspace; no state advance in the sampler
        VILA_TRY(launch_sample_batch(pick_src, m.vocab, n, m.vocab, *sampling, 0, b.pos_rows, b.draws, b.smp_ws, nullptr, nullptr, nullptr, nullptr, 0, s, any_k));
        hipLaunchKernelGGL(bver_accept_draws_kernel, dim3(1), dim3(64), 0, s, (const int64_t*)b.draws, n, st.token, st.n_draft, st.pos, st.out_ids, st.n_out,
                           st.max_out, st.hist, st.n_hist, st.hist_cap, st.n_accept);
        VILA_LAUNCH_CHECK();
    } else {
        if (pick_src == st.logits) {
            hipLaunchKernelGGL(bdec_pick1_kernel, dim3(PICK_SLICES, n), dim3(256), 0, s, st.logits, m.vocab, b.pick_v, b.pick_i);
            VILA_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(bver_accept_kernel, dim3(1), dim3(64 * n), 0, s, b.pick_v, b.pick_i, n, st.token, st.n_draft, st.pos, st.out_ids, st.n_out, st.max_out,
                           st.hist, st.n_hist, st.hist_cap, st.n_accept);
        VILA_LAUNCH_CHECK();
    }
    // behind the accept: the commit of what the step consumed, and the records of what it emitted
    if (pen != nullptr || con != nullptr)
        VILA_TRY(launch_verify_commit(pen != nullptr ? pen->counts : nullptr, m.vocab, con != nullptr ? con->state : nullptr, pb.consumed, pb.states, st.n_accept, n, s));
    if (lp) {
        VILA_TRY(launch_logprobs_verify_index(st.out_ids, st.n_out, st.n_accept, n, st.max_out, pb.tok_rows, pb.rec_rows, s));
        VILA_TRY(launch_logprobs(st.logits, m.vocab, n, m.vocab, pb.tok_rows, proc->lp_top != nullptr ? LP_TOP : 0, pb.rec_rows, 0, proc->lp_tok, proc->lp_top,
                                 proc->lp_id, proc->lp_max_rec, pb.lp_ws, s, true));
    }
    return 0;
}

// ---- operator entries of the skinny GEMM (include/vila_hip.h; tests/test_gpu_batch_gemm_elements.py) -----------------------------------
// The step's own launcher on caller-owned buffers: a BGemmArgs filled from the arguments, launch_bgemm unchanged.  What the step guarantees
// by construction (row strides that hold a row, gate/up without bias or residual, heads that exist) is refused here before anything is launched.
extern "C" int vila_gemm_batch_bf16(const void* x, int64_t ldx, int n, const void* W, const void* W2, const void* bias, const void* residual, int64_t ldr,
                                    void* y, int64_t ldy, float* y_f32, int64_t ldf, int N, int K, vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && W != nullptr, "vila_gemm_batch_bf16: NULL operand");
    VILA_REQUIRE(y != nullptr || y_f32 != nullptr, "vila_gemm_batch_bf16: NULL output (y, y_f32 or both)");
    VILA_REQUIRE(N > 0 && K > 0 && ldx >= K && (y == nullptr || ldy >= N) && (y_f32 == nullptr || ldf >= N) && (residual == nullptr || ldr >= N),
                 "vila_gemm_batch_bf16: a row stride shorter than its row (N=%d, K=%d)", N, K);
    VILA_REQUIRE(W2 == nullptr || (bias == nullptr && residual == nullptr && y_f32 == nullptr),
                 "vila_gemm_batch_bf16: gate/up takes no bias, residual or fp32 output");
    VILA_REQUIRE(residual == nullptr || y != nullptr, "vila_gemm_batch_bf16: the residual is added to the bf16 output only");
    BGemmArgs g{};
    g.x = (const bf16_t*)x; g.ldx = ldx; g.W = (const bf16_t*)W; g.W2 = (const bf16_t*)W2; g.bias = (const bf16_t*)bias;
    g.residual = (const bf16_t*)residual; g.ldr = ldr; g.y = (bf16_t*)y; g.ldy = ldy; g.y_f32 = y_f32; g.ldf = ldf;
    g.n = n; g.N = N; g.K = K; g.mode = W2 != nullptr ? 1 : 0;
    return launch_bgemm(g, vila_stream_enter((void*)stream));
}
extern "C" int vila_qkv_batch_bf16(const void* x, int64_t ldx, int n, const void* Wqkv, const void* bias, void* q_out, int64_t ldq, void* kcache, void* vcache,
                                   int64_t slot_stride, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads, int head_dim, int max_ctx, int K,
                                   vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && Wqkv != nullptr && q_out != nullptr && kcache != nullptr && vcache != nullptr && pos != nullptr && rope_cs != nullptr,
                 "vila_qkv_batch_bf16: NULL pointer");
    VILA_REQUIRE(q_heads > 0 && kv_heads > 0 && head_dim > 0 && max_ctx > 0 && K > 0 && ldx >= K && ldq >= (int64_t)q_heads * head_dim && slot_stride >= 0,
                 "vila_qkv_batch_bf16: q_heads=%d, kv_heads=%d, head_dim=%d, max_ctx=%d, or a row stride shorter than its row", q_heads, kv_heads, head_dim, max_ctx);
    BGemmArgs g{};
    g.x = (const bf16_t*)x; g.ldx = ldx; g.W = (const bf16_t*)Wqkv; g.bias = (const bf16_t*)bias;
    g.n = n; g.N = (q_heads + 2 * kv_heads) * head_dim; g.K = K; g.mode = 2;
    g.q_out = (bf16_t*)q_out; g.ldq = ldq; g.kcache = (bf16_t*)kcache; g.vcache = (bf16_t*)vcache; g.slot_stride = slot_stride;
    g.pos = pos; g.rope_cs = rope_cs; g.nq = q_heads; g.nkv = kv_heads; g.hd = head_dim; g.max_ctx = max_ctx;
    return launch_bgemm(g, vila_stream_enter((void*)stream));
}

// The same launches with the fp32 addend of a step with per-row adapters (lora_decode.hip): addend [n][N] (gate/up: [n][2 N], gate | up; row stride
// lda) joins the fp32 sum in front of the bias; a row with row_adapter[m] < 0 skips the add (row_adapter NULL: every row adds).  addend == NULL
// launches the kernels of the entries above.
extern "C" int vila_gemm_batch_lora_bf16(const void* x, int64_t ldx, int n, const void* W, const void* bias, const void* residual, int64_t ldr, void* y, int64_t ldy,
                                         float* y_f32, int64_t ldf, int N, int K, const float* addend, int64_t lda, const int32_t* row_adapter,
                                         vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && W != nullptr, "vila_gemm_batch_lora_bf16: NULL operand");
    VILA_REQUIRE(y != nullptr || y_f32 != nullptr, "vila_gemm_batch_lora_bf16: NULL output (y, y_f32 or both)");
    VILA_REQUIRE(N > 0 && K > 0 && ldx >= K && (y == nullptr || ldy >= N) && (y_f32 == nullptr || ldf >= N) && (residual == nullptr || ldr >= N),
                 "vila_gemm_batch_lora_bf16: a row stride shorter than its row (N=%d, K=%d)", N, K);
    VILA_REQUIRE(residual == nullptr || y != nullptr, "vila_gemm_batch_lora_bf16: the residual is added to the bf16 output only");
    BGemmArgs g{};
    g.x = (const bf16_t*)x; g.ldx = ldx; g.W = (const bf16_t*)W; g.bias = (const bf16_t*)bias;
    g.residual = (const bf16_t*)residual; g.ldr = ldr; g.y = (bf16_t*)y; g.ldy = ldy; g.y_f32 = y_f32; g.ldf = ldf;
    g.n = n; g.N = N; g.K = K; g.mode = 0; g.addend = addend; g.lda = lda; g.row_adapter = row_adapter;
    return launch_bgemm(g, vila_stream_enter((void*)stream));
}
extern "C" int vila_gateup_batch_lora_bf16(const void* x, int64_t ldx, int n, const void* Wgate, const void* Wup, void* y, int64_t ldy, int N, int K,
                                           const float* addend, int64_t lda, const int32_t* row_adapter, vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && Wgate != nullptr && Wup != nullptr && y != nullptr, "vila_gateup_batch_lora_bf16: NULL pointer");
    VILA_REQUIRE(N > 0 && K > 0 && ldx >= K && ldy >= N, "vila_gateup_batch_lora_bf16: a row stride shorter than its row (N=%d, K=%d)", N, K);
    BGemmArgs g{};
    g.x = (const bf16_t*)x; g.ldx = ldx; g.W = (const bf16_t*)Wgate; g.W2 = (const bf16_t*)Wup; g.y = (bf16_t*)y; g.ldy = ldy;
    g.n = n; g.N = N; g.K = K; g.mode = 1; g.addend = addend; g.lda = lda; g.row_adapter = row_adapter;
    return launch_bgemm(g, vila_stream_enter((void*)stream));
}
extern "C" int vila_qkv_batch_lora_bf16(const void* x, int64_t ldx, int n, const void* Wqkv, const void* bias, void* q_out, int64_t ldq, void* kcache, void* vcache,
                                        int64_t slot_stride, const int32_t* pos, const float* rope_cs, int q_heads, int kv_heads, int head_dim, int max_ctx, int K,
                                        const float* addend, int64_t lda, const int32_t* row_adapter, vila_stream_t stream) {
    VILA_REQUIRE(x != nullptr && Wqkv != nullptr && q_out != nullptr && kcache != nullptr && vcache != nullptr && pos != nullptr && rope_cs != nullptr,
                 "vila_qkv_batch_lora_bf16: NULL pointer");
    VILA_REQUIRE(q_heads > 0 && kv_heads > 0 && head_dim > 0 && max_ctx > 0 && K > 0 && ldx >= K && ldq >= (int64_t)q_heads * head_dim && slot_stride >= 0,
                 "vila_qkv_batch_lora_bf16: q_heads=%d, kv_heads=%d, head_dim=%d, max_ctx=%d, or a row stride shorter than its row", q_heads, kv_heads, head_dim, max_ctx);
    BGemmArgs g{};
    g.x = (const bf16_t*)x; g.ldx = ldx; g.W = (const bf16_t*)Wqkv; g.bias = (const bf16_t*)bias;
    g.n = n; g.N = (q_heads + 2 * kv_heads) * head_dim; g.K = K; g.mode = 2;
    g.q_out = (bf16_t*)q_out; g.ldq = ldq; g.kcache = (bf16_t*)kcache; g.vcache = (bf16_t*)vcache; g.slot_stride = slot_stride;
    g.pos = pos; g.rope_cs = rope_cs; g.nq = q_heads; g.nkv = kv_heads; g.hd = head_dim; g.max_ctx = max_ctx;
    g.addend = addend; g.lda = lda; g.row_adapter = row_adapter;
    return launch_bgemm(g, vila_stream_enter((void*)stream));
}

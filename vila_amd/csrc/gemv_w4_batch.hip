// W4A16 batched decode GEMV: Y[m][N] = X[m][K] . W^T for 1 <= n <= 16 activation rows on the int4 buffers of quant.py (tile_w4 / W4Weights,
// layout: gemv_w4.hip header), so one packed copy serves the solo decode, the prefill and the batched decode.
//
// The unpacked (128 + q) pairs are the B fragment of v_mfma_f32_16x16x32_bf16 exactly as in gemv_w4; where gemv_w4 broadcasts its one
// activation to all 16 A rows, here A row m is sequence m (rows m >= n are zero).  The matrix-core work per weight is the solo GEMV's and it
// serves 16 sequences instead of 1.  Numerics are gemv_w4's, per row:  acc[m][n] += scale[n] * (D[m][n] - (128 + zero[n]) * sum_group x[m]);
// the group sums come out of the matrix core too (4 more MFMAs per group with an all-ones B fragment, shared by every tile of the wave),
// already in the C layout (sequence lg*4 + r, feature l15).  The weights are never dequantised.
//
// Activations: gemv_w4 stages all of x in LDS, which at 16 rows x K = 18944 is 606 KB.  Here a wave holds the A fragments of the groups it
// is working on in registers (lane (m, g) reads 64 contiguous bytes of row m per group from L2, where the activations live: <= 606 KB) and
// reuses them for its T tiles.  Per group a 16-row weight tile is 1 KB of int4 and the 16 activation rows are 4 KB, so T = 4 (gate/up)
// moves as many activation bytes through L2 as weight bytes, where a wave per tile would move four times as many.
// Work split: a block owns T consecutive 16-row tiles, its W waves split K into contiguous group ranges, and the W partial sums meet in LDS
// in wave order (fixed order, no atomics: bit-identical from run to run and between graph replay and eager launches).  Grids of few tiles
// (o_proj / down_proj: 224 tiles at NVILA-8B) take T = 1 so every CU has a tile, as gemv_w4 does.
//
// Epilogues mirror decode_batch.hip's bgemm_epilogue rounding on W4Weights' packed row orders: 0 plain (+bias)(+residual; y may alias the
// residual), 1 gate/up (packed rows 2i, 2i + 1 -> silu(g) * u), 2 q|k|v (q and k heads RoPE-interleaved: bias, RoPE at the row's own position,
// q to q_out[m] in natural order, K/V appended into row m's cache slot at pos[m], skipped when pos[m] >= max_ctx).
#include "gemv_common.h"
#include "w4.h"

#define W4B_MAX_WAVES 16
#define W4B_MAX_T 4

// T = 1 blocks take up to 16 waves (K split of down_proj); blocks of several tiles up to 8 (more VGPRs for the T x UB weight loads in flight)
template <int MODE, int T, int UB>
__global__ __launch_bounds__(T == 1 ? 1024 : 512) void gemv_w4_batch_kernel(GemvW4BatchArgs p, int n_tiles, int n_items) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, W = blockDim.x >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int G = p.K >> 7;
    const int g0 = (G * wv) / W, g1 = (G * (wv + 1)) / W;
    const bool a_live = l15 < p.n;                                     // A row l15 is a sequence of the batch
    const bf16_t* xrow = p.x + (int64_t)(a_live ? l15 : 0) * p.ldx + lg * 32;
    const u32x4* wq_base = (const u32x4*)p.Wq + lane;
    const uint32_t* wsz_base = p.Wsz + l15;
    const u32x4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};      // bf16 1.0 pairs: D = the group sums of x
    float* red_base = (float*)smem;                                    // [2 parities][W][T][64 lanes][4]
    int par = 0;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {     // block-uniform
        const int tile0 = item * T;
        f32x4 total[T];
#pragma unroll
        for (int t = 0; t < T; ++t) total[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int gb = g0; gb < g1; gb += UB) {
            u32x4 wr[T][UB], xa[UB][4];
            uint32_t sr[T][UB];
            // everything of the batch is issued before anything is used: T x UB weight loads (1 KB each) and UB activation groups
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int c = gb + u;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const bool ok = c < g1 && tile0 + t < n_tiles;
                    const size_t tg = (size_t)(tile0 + t) * G + c;
                    wr[t][u] = ok ? __builtin_nontemporal_load(wq_base + tg * 64) : (u32x4){0u, 0u, 0u, 0u};
                    sr[t][u] = ok ? __builtin_nontemporal_load(wsz_base + tg * 16) : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int c = gb + u;
                const bool ok = c < g1 && a_live;
#pragma unroll
                for (int w = 0; w < 4; ++w) xa[u][w] = ok ? *(const u32x4*)(xrow + c * 128 + w * 8) : (u32x4){0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                if (gb + u < g1) {                                     // wave-uniform
                    f32x4 sx = (f32x4){0.f, 0.f, 0.f, 0.f}, d[T];
#pragma unroll
                    for (int t = 0; t < T; ++t) d[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const bf16x8 a = __builtin_bit_cast(bf16x8, xa[u][w]);
                        sx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8, ones), sx, 0, 0, 0);
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            const uint32_t q = wr[t][u][w];
                            u32x4 b;
#pragma unroll
                            for (int j = 0; j < 4; ++j) b[j] = ((q >> (4 * j)) & 0x000F000Fu) | 0x43004300u;
                            d[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8, b), d[t], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const float sc = lo_bf(sr[t][u]), zp = hi_bf(sr[t][u]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) total[t][r] = fmaf(sc, d[t][r] - zp * sx[r], total[t][r]);
                    }
                }
            }
        }
        // ---- the W partial sums meet in LDS (double-buffered: one barrier per item) ----
        float* rd = red_base + par * (W * T * 256);
        par ^= 1;
#pragma unroll
        for (int t = 0; t < T; ++t) *(f32x4*)(rd + ((wv * T + t) * 64 + lane) * 4) = total[t];
        __syncthreads();
        for (int e = tid; e < T * 256; e += blockDim.x) {
            const int t = e >> 8, m = (e >> 4) & 15, n = e & 15;
            const int tile = tile0 + t;
            if (m >= p.n || tile >= n_tiles) continue;
            // C layout: sequence m = lg*4 + r, feature n = l15
            const int o_own = ((m >> 2) * 16 + n) * 4 + (m & 3), o_par = ((m >> 2) * 16 + (n ^ 1)) * 4 + (m & 3);
            float v = 0.f, vp = 0.f;
            for (int w = 0; w < W; ++w) {
                const float* rw = rd + (w * T + t) * 256;
                v += rw[o_own];
                vp += rw[o_par];
            }
            const int pr = tile * 16 + n;                              // packed row
            if constexpr (MODE == 0) {
                if (pr < p.N) {
                    v += p.bias != nullptr ? bf2f(p.bias[pr]) : 0.f;
                    if (p.residual != nullptr) v = bfround(v) + bf2f(p.residual[(int64_t)m * p.ldr + pr]);
                    p.y[(int64_t)m * p.ldy + pr] = f2bf(v);
                }
            } else if constexpr (MODE == 1) {
                if ((n & 1) == 0 && (pr >> 1) < p.N) p.y[(int64_t)m * p.ldy + (pr >> 1)] = f2bf(bfround(silu_f(bfround(v))) * bfround(vp));
            } else {
                const int half = p.hd >> 1;
                const int head = pr / p.hd, within = pr - head * p.hd;
                if (head >= p.nq + 2 * p.nkv) continue;
                const bool is_v = head >= p.nq + p.nkv;
                int d;                                                 // element of the head this thread produces
                float out;
                if (is_v) {
                    d = within;
                    out = bfround(v + (p.bias != nullptr ? bf2f(p.bias[pr]) : 0.f));
                } else {
                    const int i = within >> 1, b = within & 1;
                    d = i + b * half;
                    const float e0 = p.bias != nullptr ? bf2f(p.bias[head * p.hd + i + b * half]) : 0.f;
                    const float e1 = p.bias != nullptr ? bf2f(p.bias[head * p.hd + i + (b ^ 1) * half]) : 0.f;
                    const float c = p.rope_cs[m * p.hd + i], sn = p.rope_cs[m * p.hd + half + i];
                    const float mine = bfround(v + e0), other = bfround(vp + e1);
                    // rotate-half: lo' = lo*c - hi*s ; hi' = hi*c + lo*s   (bf16 rounding after every op, as bgemm_epilogue)
                    out = b ? bfround(bfround(mine * c) + bfround(other * sn)) : bfround(bfround(mine * c) + bfround(-other * sn));
                }
                if (head < p.nq) {
                    p.q_out[(int64_t)m * p.ldq + head * p.hd + d] = f2bf(out);
                } else {
                    const int ps = p.pos[m];
                    if (ps < p.max_ctx) {
                        const int kvh = is_v ? head - p.nq - p.nkv : head - p.nq;
                        bf16_t* dst = (is_v ? p.vcache : p.kcache) + (int64_t)m * p.slot_stride + ((int64_t)kvh * p.max_ctx + ps) * p.hd;
                        dst[d] = f2bf(out);
                    }
                }
            }
        }
    }
}

template <int MODE, int T>
static int launch_w4b_t(const GemvW4BatchArgs& a, int n_tiles, int W, hipStream_t s) {
    constexpr int UB = T == 4 ? 2 : 4;                                 // groups per load batch: ~100 VGPRs at every T
    const int n_items = cdiv(n_tiles, T);
    const size_t lds = (size_t)2 * W * T * 256 * 4;
    static bool attr = false;
    if (!attr) {
        VILA_HIP(hipFuncSetAttribute((const void*)gemv_w4_batch_kernel<MODE, T, UB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)((size_t)2 * W4B_MAX_WAVES * W4B_MAX_T * 256 * 4)));
        attr = true;
    }
    // persistent blocks: at most as many as are resident at once (<= 128 VGPRs at T = 1: 16 waves per CU; <= 168 above: 12), each walks
    // items blockIdx, + grid, ...
    const int resident = 256 * ((T == 1 ? 16 : 12) / W);
    const int grid = n_items < resident ? n_items : resident;
    hipLaunchKernelGGL((gemv_w4_batch_kernel<MODE, T, UB>), dim3(grid), dim3(W * 64), lds, s, a, n_tiles, n_items);
    VILA_LAUNCH_CHECK();
    return 0;
}

int launch_gemv_w4_batch(const GemvW4BatchArgs& a, hipStream_t s) {
    VILA_REQUIRE(a.n >= 1 && a.n <= 16, "gemv_w4_batch: 1..16 activation rows (got %d)", a.n);
    VILA_REQUIRE(a.K % 128 == 0 && a.K > 0 && a.N > 0, "gemv_w4_batch: K=%d must be a positive multiple of the 128-wide quantisation group", a.K);
    VILA_REQUIRE(a.x != nullptr && a.Wq != nullptr && a.Wsz != nullptr, "gemv_w4_batch: NULL operand");
    VILA_REQUIRE((uintptr_t)a.x % 16 == 0 && (uintptr_t)a.Wq % 16 == 0 && a.ldx % 8 == 0 && a.ldx >= a.K, "gemv_w4_batch: operand alignment");
    int rows = a.N;                                                    // packed rows
    if (a.mode == 0) {
        VILA_REQUIRE(a.y != nullptr && a.ldy >= a.N && (a.residual == nullptr || a.ldr >= a.N), "gemv_w4_batch: plain mode needs y");
    } else if (a.mode == 1) {
        VILA_REQUIRE(a.y != nullptr && a.ldy >= a.N && a.bias == nullptr && a.residual == nullptr,
                     "gemv_w4_batch: gate/up mode needs y and takes no bias or residual");
        rows = 2 * a.N;
    } else if (a.mode == 2) {
        VILA_REQUIRE(a.hd % 16 == 0 && a.hd > 0 && a.N == (a.nq + 2 * a.nkv) * a.hd && a.q_out && a.kcache && a.vcache && a.pos && a.rope_cs &&
                     a.ldq >= a.nq * a.hd, "gemv_w4_batch: q|k|v mode needs head_dim %% 16 == 0, N = (q + 2 kv) heads and its outputs");
    } else {
        VILA_REQUIRE(false, "gemv_w4_batch: mode must be 0 (plain), 1 (gate/up) or 2 (q|k|v), got %d", a.mode);
    }
    const int G = a.K / 128;
    const int n_tiles = cdiv(rows, 16);
    // K split: W waves of ~7 groups (K = 3584 -> 4 waves; K = 18944 -> 16 waves of 9-10 groups)
    // tiles per block: activation reuse where the grid stays full, one tile per block where there are fewer tiles than 2 per CU
    const int T = n_tiles >= 1024 ? 4 : (n_tiles >= 512 ? 2 : 1);
    const int max_w = T == 1 ? W4B_MAX_WAVES : W4B_MAX_WAVES / 2;
    int W = cdiv(G, 7);
    W = W < 1 ? 1 : (W > max_w ? max_w : W);
#define W4B_LAUNCH(MODE_) (T == 4 ? launch_w4b_t<MODE_, 4>(a, n_tiles, W, s) : T == 2 ? launch_w4b_t<MODE_, 2>(a, n_tiles, W, s) : launch_w4b_t<MODE_, 1>(a, n_tiles, W, s))
    if (a.mode == 1) return W4B_LAUNCH(1);
    if (a.mode == 2) return W4B_LAUNCH(2);
    return W4B_LAUNCH(0);
#undef W4B_LAUNCH
}

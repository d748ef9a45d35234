// W4A16 GEMM for prefill shapes (SURVEY.md §8f row 3 / BASELINE configs[4]):  Y[M, N] = X[M, K] . W4^T, any M >= 1.
// Tests: every element in tests/test_gpu_w4_elements.py (bit for bit on exact inputs, a derived bound otherwise; tests/test_w4_bound_cpu.py proves both).
// W4 is the SAME tile-major buffer the decode GEMVs read (gemv_w4.hip header, vila_amd/quant.py tile_w4): one packed copy serves both.
// That layout already is the B operand of v_mfma_f32_16x16x32_bf16: lane 16g + n of a 16-row tile holds k = 32g .. 32g+31 of row n
// for one 128-wide group, and word w of the lane, unpacked with ((word >> 4p) & 0x000F000F) | 0x43004300 into the exact bf16 pairs
// 128 + q, is the B fragment of MFMA number w.  So the A fragment of lane (m, g) for MFMA w is X[m][32g + 8w .. +7]: per group a lane
// reads 64 contiguous bytes of its activation row from LDS.
//
// Numerics as gemv_w4.hip: per group D[m][n] = sum_k x[m][k] (128 + q[n][k]) on the matrix cores, then in fp32
//   acc[m][n] += scale[n] * (D[m][n] - (128 + zero[n]) * sum_group x[m])
// with the group sums taken from the staged bf16 tile.  The weights are never dequantised to bf16 (that would add a rounding the fp32
// dequantise-then-matmul oracle does not have).
//
// Block = 4 waves, tile 64 rows (M) x 128 packed rows (N, 8 weight tiles); wave w owns weight tiles 2w, 2w+1 for all 64 rows (4 x 2
// accumulators of 16 x 16).  Per group the block stages X[64][128] into LDS (double-buffered, the next group is loaded into registers
// while the current one is multiplied; rows padded by 16 B so the 16 rows of a fragment read fall into different banks) and each wave
// loads its two 1-KB weight tiles straight into registers (one group ahead).  Blocks walk M fastest, so the blocks that share a weight
// tile run together and the weights come from HBM about once.
//
// Under-filled grids (small M: prompts of a few dozen tokens) are sliced over K: each slice writes an fp32 slab [slice][M][packed rows],
// and a second kernel adds the slabs in slice order and applies the epilogue.  No atomics anywhere: the result is bit-identical from
// run to run.
//
// Epilogues (packed-row orders of quant.py W4Weights):
//   0 plain     y = W x (+bias)(+residual), residual rounded like gemv_w4 mode 0 (o_proj / down_proj: x += W h, y may alias residual)
//   1 gate/up   rows 2i / 2i+1 = gate i / up i (neighbouring lanes of the C layout): y[m][i] = silu(g) * u, rounded as gemv_w4 mode 1
//   2 qkv       q and k heads RoPE-interleaved (quant.py rope_interleave_rows): written back in natural column order with the bias
//               added, exactly what the bf16 q|k|v GEMM leaves for rope_kv_kernel
#include "w4.h"

namespace {
constexpr int BM = 64, BN = 128, THREADS = 256;
constexpr int SROW = 128 + 8;                      // LDS row of the staged activation: 128 bf16 + 16 B pad
constexpr int MAX_SPLITS = 8;

struct Geo { int mt, nt, splits, prows; };

Geo geometry(int M, int N, int K, int mode) {
    Geo g;
    g.prows = mode == 1 ? 2 * N : N;
    g.mt = cdiv(M, BM);
    g.nt = cdiv(g.prows, BN);
    const int G = K / 128, blocks = g.mt * g.nt;
    // one round of the chip (256 CUs) at least, where K allows it
    int sp = blocks >= 256 ? 1 : cdiv(256, blocks);
    if (sp > MAX_SPLITS) sp = MAX_SPLITS;
    if (sp > G) sp = G;
    g.splits = sp;
    return g;
}

// the epilogue of one output element pair: v = packed row pr, vp = the partner row pr ^ 1 (gate/up)
__device__ __forceinline__ void store_out(const GemmW4Args& p, int m, int pr, float v, float vp) {
    if (p.mode == 1) {
        if ((pr & 1) == 0) p.y[(size_t)m * p.N + (pr >> 1)] = f2bf(bfround(silu_f(bfround(v))) * bfround(vp));
    } else if (p.mode == 2) {
        int col = pr;
        const int head = pr / p.hd;
        if (head < p.n_rope_heads) {
            const int within = pr - head * p.hd;
            col = head * p.hd + (within >> 1) + (within & 1) * (p.hd >> 1);
        }
        if (p.bias != nullptr) v += bf2f(p.bias[col]);
        p.y[(size_t)m * p.N + col] = f2bf(v);
    } else {
        const size_t o = (size_t)m * p.N + pr;
        if (p.bias != nullptr) v += bf2f(p.bias[pr]);
        if (p.residual != nullptr) v = bfround(v) + bf2f(p.residual[o]);
        p.y[o] = f2bf(v);
    }
}

__global__ __launch_bounds__(THREADS) void gemm_w4_kernel(GemmW4Args p, int mt, int nt, int splits, int prows, float* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) bf16_t sx[2][BM * SROW];
    __shared__ __attribute__((aligned(16))) float xg[2][BM];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = p.K, G = K >> 7, M = p.M;
    int bid = blockIdx.x;
    const int bm = bid % mt; bid /= mt;
    const int bn = bid % nt;
    const int sl = bid / nt;
    const int g0 = (G * sl) / splits, g1 = (G * (sl + 1)) / splits;
    const int m0 = bm * BM;
    const int n_tiles = prows >> 4;
    const int tile0 = bn * (BN / 16) + 2 * wv;                 // this wave's two weight tiles
    const bool have[2] = {tile0 < n_tiles, tile0 + 1 < n_tiles};

    // activation staging: thread t moves chunks c = t + 256 i (8 bf16 each) of the [64][128] group tile; 16 consecutive lanes = one row
    u32x4 ar[4];
    auto load_a = [&](int grp) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + THREADS * i, r = c >> 4, kc = c & 15;
            ar[i] = (m0 + r < M) ? *(const u32x4*)(p.x + (size_t)(m0 + r) * K + grp * 128 + kc * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + THREADS * i, r = c >> 4, kc = c & 15;
            *(u32x4*)(&sx[buf][r * SROW + kc * 8]) = ar[i];
            const u32x4 t = ar[i];
            float a = ((lo_bf(t[0]) + hi_bf(t[0])) + (lo_bf(t[1]) + hi_bf(t[1]))) + ((lo_bf(t[2]) + hi_bf(t[2])) + (lo_bf(t[3]) + hi_bf(t[3])));
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) a += __shfl_xor(a, o, 64);
            if (kc == 0) xg[buf][r] = a;
        }
    };
    // weights: one 16-B fragment per lane and tile, the lane's {scale, 128 + zero} word
    const u32x4* wq = (const u32x4*)p.Wq + lane;
    const uint32_t* wsz = p.Wsz + (lane & 15);
    u32x4 bw[2], bw_n[2];
    uint32_t bs[2], bs_n[2];
    auto load_b = [&](int grp, u32x4 (&w)[2], uint32_t (&s)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            w[j] = have[j] ? wq[((size_t)(tile0 + j) * G + grp) * 64] : (u32x4){0u, 0u, 0u, 0u};
            s[j] = have[j] ? wsz[((size_t)(tile0 + j) * G + grp) * 16] : 0u;
        }
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_a(g0);
    load_b(g0, bw, bs);
    store_a(0);
    __syncthreads();
    const int g = lane >> 4, mrow = lane & 15;
    for (int grp = g0, buf = 0; grp < g1; ++grp, buf ^= 1) {
        const bool next = grp + 1 < g1;                         // block-uniform
        if (next) { load_a(grp + 1); load_b(grp + 1, bw_n, bs_n); }
        f32x4 d[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) d[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const bf16_t* xa = &sx[buf][mrow * SROW + g * 32];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            u32x4 b[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) b[j][q] = ((bw[j][w] >> (4 * q)) & 0x000F000Fu) | 0x43004300u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u32x4 a = *(const u32x4*)(xa + i * 16 * SROW + w * 8);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    d[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b[j]), d[i][j], 0, 0, 0);
            }
        }
        // the 128- and zero-offsets come out per group: C row = 4 (lane >> 4) + r of each 16-row subtile, column = lane & 15
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 s = *(const f32x4*)(&xg[buf][i * 16 + 4 * g]);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float sc = lo_bf(bs[j]), zp = hi_bf(bs[j]);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = fmaf(sc, d[i][j][r] - zp * s[r], acc[i][j][r]);
            }
        }
        if (next) {
            store_a(buf ^ 1);
#pragma unroll
            for (int j = 0; j < 2; ++j) { bw[j] = bw_n[j]; bs[j] = bs_n[j]; }
        }
        __syncthreads();
    }

    // output: lane holds rows m0 + 16 i + 4 g + r of packed rows 16 tile + (lane & 15)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[i][j][r];
                const float vp = __shfl_xor(v, 1, 64);          // the gate/up partner (every lane takes part)
                const int m = m0 + i * 16 + 4 * g + r, pr = (tile0 + j) * 16 + (lane & 15);
                if (!have[j] || m >= M) continue;
                if (splits > 1) slab[((size_t)sl * M + m) * prows + pr] = v;
                else store_out(p, m, pr, v, vp);
            }
}

// slices in order -> epilogue; one thread per (row, packed row pair)
__global__ __launch_bounds__(256) void gemm_w4_reduce_kernel(GemmW4Args p, int splits, int prows, const float* __restrict__ slab) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int half = prows >> 1;
    if (idx >= (int64_t)p.M * half) return;
    const int m = (int)(idx / half), pr = 2 * (int)(idx - (int64_t)m * half);
    const size_t plane = (size_t)p.M * prows;
    const float* s = slab + (size_t)m * prows + pr;
    float v0 = 0.f, v1 = 0.f;
    for (int k = 0; k < splits; ++k) { v0 += s[k * plane]; v1 += s[k * plane + 1]; }
    store_out(p, m, pr, v0, v1);
    if (p.mode != 1) store_out(p, m, pr + 1, v1, v0);
}
}  // namespace

size_t gemm_w4_workspace_bytes(int M, int N, int K, int mode) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 128 != 0) return 0;
    const Geo g = geometry(M, N, K, mode);
    return g.splits > 1 ? align_up((size_t)g.splits * M * g.prows * 4, 256) : 0;
}

int launch_gemm_w4(const GemmW4Args& a, void* ws, size_t ws_bytes, hipStream_t s) {
    VILA_REQUIRE(a.M > 0 && a.N > 0, "gemm_w4: empty problem (M=%d, N=%d)", a.M, a.N);
    VILA_REQUIRE(a.K > 0 && a.K % 128 == 0, "gemm_w4: K=%d must be a multiple of the 128-wide quantisation group", a.K);
    VILA_REQUIRE(a.N % 16 == 0, "gemm_w4: N=%d must be a multiple of the 16-row weight tile", a.N);
    VILA_REQUIRE(a.mode >= 0 && a.mode <= 2, "gemm_w4: mode %d is not 0 (plain), 1 (gate/up) or 2 (qkv)", a.mode);
    VILA_REQUIRE(a.x != nullptr && a.Wq != nullptr && a.Wsz != nullptr && a.y != nullptr, "gemm_w4: NULL pointer");
    VILA_REQUIRE((uintptr_t)a.x % 16 == 0 && (uintptr_t)a.Wq % 16 == 0, "gemm_w4: x and Wq must be 16-byte aligned");
    VILA_REQUIRE(a.mode == 0 || a.residual == nullptr, "gemm_w4: a residual is only taken by the plain mode (mode %d)", a.mode);
    VILA_REQUIRE(a.mode != 1 || a.bias == nullptr, "gemm_w4: the gate/up mode takes no bias");
    if (a.mode == 2)
        VILA_REQUIRE(a.hd > 0 && a.hd % 16 == 0 && a.n_rope_heads >= 0 && a.n_rope_heads * a.hd <= a.N,
                     "gemm_w4: qkv mode needs head_dim (%d) a multiple of 16 and n_rope_heads * head_dim <= N", a.hd);
    const Geo g = geometry(a.M, a.N, a.K, a.mode);
    const size_t need = gemm_w4_workspace_bytes(a.M, a.N, a.K, a.mode);
    VILA_REQUIRE(ws_bytes >= need && (need == 0 || ws != nullptr), "gemm_w4: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    const int64_t blocks = (int64_t)g.mt * g.nt * g.splits;
    VILA_REQUIRE(blocks < (1ll << 31), "gemm_w4: grid too large");
    float* slab = g.splits > 1 ? (float*)ws : nullptr;
    hipLaunchKernelGGL(gemm_w4_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, a, g.mt, g.nt, g.splits, g.prows, slab);
    VILA_LAUNCH_CHECK();
    if (g.splits > 1) {
        const int64_t pairs = (int64_t)a.M * (g.prows / 2);
        hipLaunchKernelGGL(gemm_w4_reduce_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, a, g.splits, g.prows, (const float*)slab);
        VILA_LAUNCH_CHECK();
    }
    return 0;
}

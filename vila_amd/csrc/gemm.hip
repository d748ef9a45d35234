// bf16 MFMA GEMM for the prefill / ViT / projector / lm_head contractions and the dgrad / wgrad GEMMs of the SFT step
// (SURVEY.md §8 rows a2,a3,a5,a10,a11,a13).
//
//   C[M,N] = epi(A[M,K] . W[N,K]^T + bias) (+ residual)        nn.Linear layout: W is [out,in] row-major,
//   so BOTH operands are K-contiguous = the natural MFMA A/B fragment layout (8 consecutive k per lane).
//
// One kernel template, three tile shapes (waves are WM x 2, each wave owns 64 x (16*NF) of C as 4 x NF
// v_mfma_f32_16x16x32_bf16 fragments, K-tile 64):
//     256 x 128  (8 waves)  M >= 1536: SFT-step shapes; halves the B-tile bytes per flop (the 128^2 tile is exactly
//                           L1/LDS-bound on gfx950: 32 KB per K-tile at 64 B/clk == its 512 MFMA cycles)
//     128 x 128  (4 waves)  default
//     128 x  64  (4 waves)  small grids (S = 769 prefill with N <= 4608: 196 tiles of 128^2 cannot fill 256 CUs)
// HBM -> registers -> LDS (XOR-swizzled 16-B slots, double buffered, one barrier per K-tile; loads for tile t+1 are
// issued before the MFMAs of tile t and written to LDS after them).  The epilogue goes through LDS so that the
// residual read and the C write are full-row coalesced (8 / 16 B per lane).
// Roofline: MFMA (2*M*N*K flop vs (M+N)*K*2 + M*N*2 bytes).
#include <stdio.h>
#include <stdlib.h>
#include "kernels.h"
#include "gemm_plan.h"
#include "../../include/vila_hip_tuning.h"

#define BK 64
#define STG 68  // fp32 staging row stride (floats)

template <int EPI, bool OUT_F32, int WM, int NF>
__global__ __launch_bounds__(WM * 128, (WM == 2) ? 2 : 2) void gemm_bf16_tn(GemmArgs p, int tiles_m) {
    constexpr int THREADS = WM * 128;
    constexpr int BM = WM * 64;              // rows of C per block
    constexpr int BNT = 32 * NF;             // B-tile rows held in LDS (2 waves x 16*NF)
    constexpr int A_IT = BM * 8 / THREADS;   // 16-B chunks per thread and K-tile
    constexpr int B_IT = (BNT * 8 + THREADS - 1) / THREADS;
    constexpr int RSTEP = THREADS / 8;       // rows covered per staging pass
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* sA = (bf16_t*)smem;              // [2][BM][64]
    bf16_t* sB = sA + 2 * BM * BK;           // [2][BNT][64]
    float* stage = (float*)smem;             // epilogue reuse: [waves][64][STG]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, lg = lane >> 4;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = id % tiles_m, tn = id / tiles_m;
    constexpr int WN = 16 * NF;                                   // C columns per wave held in registers
    constexpr int WN_OUT = (EPI == EPI_GATEUP) ? WN / 2 : WN;     // C columns per wave written
    constexpr int BN_OUT = 2 * WN_OUT;
    const int m0 = tm * BM, n0 = tn * BN_OUT;
    const int M = p.M, N = p.N, K = p.K;

    // ---- staging coordinates: thread owns 16-B chunk (row = r0 + RSTEP*i, kc) ----
    const int kc = tid & 7, r0 = tid >> 3;
    const int sw = kc ^ ((r0 >> 1) & 7);     // RSTEP is a multiple of 16 => same swizzle for every pass
    const bf16_t* a_ptr[A_IT];
    const bf16_t* b_ptr[B_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        int gm = m0 + r0 + RSTEP * i; gm = gm < M ? gm : M - 1;
        a_ptr[i] = p.A + (int64_t)gm * p.lda + kc * 8;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int row = r0 + RSTEP * i;      // B-tile row: wave column = row / WN, fragment j = (row % WN) / 16
        if constexpr (EPI == EPI_GATEUP) {
            const int j = (row % WN) >> 4;
            int gn = n0 + (row / WN) * WN_OUT + (j % (NF / 2)) * 16 + (row & 15); gn = gn < N ? gn : N - 1;
            b_ptr[i] = ((j >= NF / 2) ? p.W2 : p.W) + (int64_t)gn * p.ldw + kc * 8;
        } else {
            int gn = n0 + row; gn = gn < N ? gn : N - 1;
            b_ptr[i] = p.W + (int64_t)gn * p.ldw + kc * 8;
        }
    }
    const int st_off = r0 * BK + sw * 8;
    const bool b_active = (B_IT * RSTEP == BNT) || (r0 < BNT);   // 128x64 tile with 256 threads: only half the threads stage B

    // ---- fragment read offsets (elements) ----
    const int sw_r = (l15 >> 1) & 7;
    int a_off[2], b_off[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int kcc = ks * 4 + lg;
        a_off[ks] = (wr * 64 + l15) * BK + ((kcc ^ sw_r) << 3);
        b_off[ks] = (wc * WN + l15) * BK + ((kcc ^ sw_r) << 3);
    }

    f32x4 acc[4][NF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nt = (K + BK - 1) / BK;
    u32x4 ra[A_IT], rb[B_IT];
    auto gload = [&](int t) {
        const int k0 = t * BK;
        const bool ok = (k0 + kc * 8) < K;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) ra[i] = ok ? *(const u32x4*)(a_ptr[i] + k0) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < B_IT; ++i) rb[i] = (ok && b_active) ? *(const u32x4*)(b_ptr[i] + k0) : (u32x4){0u, 0u, 0u, 0u};
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) *(u32x4*)(sA + buf * BM * BK + st_off + RSTEP * i * BK) = ra[i];
        if (b_active) {
#pragma unroll
            for (int i = 0; i < B_IT; ++i) *(u32x4*)(sB + buf * BNT * BK + st_off + RSTEP * i * BK) = rb[i];
        }
    };

    gload(0);
    lstore(0);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) gload(t + 1);
        const bf16_t* cA = sA + buf * BM * BK;
        const bf16_t* cB = sB + buf * BNT * BK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bfr[NF];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *(const bf16x8*)(cA + a_off[ks] + i * 16 * BK);
#pragma unroll
            for (int j = 0; j < NF; ++j) bfr[j] = *(const bf16x8*)(cB + b_off[ks] + j * 16 * BK);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nt) lstore(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: bias / activation in registers -> per-wave fp32 staging -> coalesced residual add + store ----
    float* wst = stage + wave * 64 * STG;
    const int ncol0 = n0 + wc * WN_OUT;
    if constexpr (EPI == EPI_GATEUP) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NF / 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float g = acc[i][j][r], u = acc[i][j + NF / 2][r];
                    wst[(i * 16 + lg * 4 + r) * STG + j * 16 + l15] = silu_f(g) * u;
                }
    } else {
        float bv[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int col = ncol0 + j * 16 + l15;
            bv[j] = (p.bias != nullptr && col < N) ? bf2f(p.bias[col]) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[i][j][r] + bv[j];
                    if constexpr (EPI == EPI_GELU_TANH) v = gelu_tanh_f(v);
                    if constexpr (EPI == EPI_GELU_ERF) v = gelu_erf_f(v);
                    wst[(i * 16 + lg * 4 + r) * STG + j * 16 + l15] = v;
                }
    }
    // each wave only reads back what it wrote itself: a wave-level LDS fence is enough
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();

    constexpr int LPR = WN_OUT / 4;      // lanes per output row
    constexpr int RPI = 64 / LPR;        // rows per pass
    const int rr0 = lane / LPR, c4 = (lane % LPR) * 4;
#pragma unroll
    for (int it = 0; it < 64 / RPI; ++it) {
        const int rr = it * RPI + rr0;
        const int gm = m0 + wr * 64 + rr, gc = ncol0 + c4;
        if (gm < M && gc < N) {
            f32x4 v = *(const f32x4*)(wst + rr * STG + c4);
            if (p.residual != nullptr) {
                const u32x2 rv = *(const u32x2*)(p.residual + (int64_t)(p.res_mod > 0 ? gm % p.res_mod : gm) * p.ldr + gc);
                v[0] += lo_bf(rv[0]); v[1] += hi_bf(rv[0]); v[2] += lo_bf(rv[1]); v[3] += hi_bf(rv[1]);
            }
            if constexpr (OUT_F32) {
                *(f32x4*)((float*)p.C + (int64_t)gm * p.ldc + gc) = v;
            } else {
                u32x2 o; o[0] = pack2bf(v[0], v[1]); o[1] = pack2bf(v[2], v[3]);
                *(u32x2*)((bf16_t*)p.C + (int64_t)gm * p.ldc + gc) = o;
            }
        }
    }
}

template <int EPI, bool OUT_F32, int WM, int NF>
static int launch_cfg(const GemmArgs& a, hipStream_t s) {
    constexpr int BM = WM * 64, BNT = 32 * NF;
    constexpr int BN_OUT = (EPI == EPI_GATEUP) ? BNT / 2 : BNT;
    const int tiles_m = cdiv(a.M, BM), tiles_n = cdiv(a.N, BN_OUT);
    const size_t lds_main = (size_t)2 * (BM + BNT) * BK * 2, lds_epi = (size_t)WM * 2 * 64 * STG * sizeof(float);
    const size_t lds = lds_main > lds_epi ? lds_main : lds_epi;
    static bool attr_set = false;
    if (!attr_set) {
        VILA_HIP(hipFuncSetAttribute((const void*)gemm_bf16_tn<EPI, OUT_F32, WM, NF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_bf16_tn<EPI, OUT_F32, WM, NF>), dim3(tiles_m * tiles_n), dim3(WM * 128), lds, s, a, tiles_m);
    VILA_LAUNCH_CHECK();
    return 0;
}

int launch_gemm256(const GemmArgs& a, const GemmPlan& p, hipStream_t s);              // gemm256.hip
int launch_gemm256_splitk(const GemmArgs& a, const GemmPlan& p, hipStream_t s);
int launch_gemm_ring(const GemmArgs& a, int ring, int pipe, hipStream_t s);           // gemm_ring.hip
int launch_gemm_ring_splitk(const GemmArgs& a, int splits, hipStream_t s);            // gemm_ring_splitk.hip

// ---- the tuning knobs (gemm_plan.h GemmKnobs): one struct, written by the hooks of vila_hip_tuning.h, its "ask the environment" values filled once ----
static GemmKnobs g_gemm_knobs;
extern "C" void vila_gemm_force_tile(int t) { g_gemm_knobs.force_tile = t; }
extern "C" void vila_gemm_force_sched(int sched) { g_gemm_knobs.sched = sched; }
extern "C" void vila_gemm_force_group(int grp) { g_gemm_knobs.group = grp; }
extern "C" void vila_gemm_force_ex(int mode) { g_gemm_knobs.ex = mode; }
extern "C" void vila_gemm_force_bm(int bm) { g_gemm_knobs.bm = bm; }
extern "C" void vila_gemm_force_hybrid(int on) { g_gemm_knobs.hybrid = on; }
extern "C" void vila_gemm_force_fuse_norm(int on) { g_gemm_knobs.fuse_norm = on ? 1 : 0; }
static const GemmKnobs& gemm_knobs() {
    GemmKnobs& k = g_gemm_knobs;
    if (k.ex < 0) { const char* e = getenv("VILA_GEMM_EX"); k.ex = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1; }
    if (k.ring_splitk < 0) { const char* e = getenv("VILA_RING_SPLITK"); k.ring_splitk = (e && e[0] == '0') ? 0 : 1; }
    if (k.ring_pipe < 0) { const char* e = getenv("VILA_RING_PIPE"); k.ring_pipe = (e && e[0] == '0') ? 0 : 2; }
    if (k.fuse_norm < 0) { const char* e = getenv("VILA_FUSE_NORM"); k.fuse_norm = (e && e[0] == '0') ? 0 : 1; }
    return k;
}

static GemmShape shape_of(const GemmArgs& a) {
    return GemmShape{a.M, a.N, a.K, a.lda, a.ldw, a.epi, a.out_f32, a.a_cm, a.b_cm, a.ws != nullptr, a.ws_bytes,
                     a.norm_out != nullptr && a.norm_w != nullptr, gemm_rope_offer(a)};
}
static bool gemm256_supported(const GemmArgs& a) { return gemm256_supported(shape_of(a)); }

// One line of text for the plan of a problem under the current knobs: host only, launches nothing and asks the runtime for no device (packed
// operands are assumed: lda / ldw = K, or the row count for a contraction-major operand).  offers: bit 0 = the next block's normalisation,
// bit 1 = the q/k/v RoPE + KV follow-up.  Returns the length written, -1 when the buffer is too small.
extern "C" int vila_gemm_plan_describe(int M, int N, int K, int epi, int out_f32, int a_cm, int b_cm, size_t ws_bytes, int offers, char* buf, int buf_len) {
    const GemmShape h{M, N, K, a_cm ? M : K, b_cm ? N : K, epi, out_f32, a_cm, b_cm, ws_bytes > 0, ws_bytes, (offers & 1) != 0, (offers & 2) != 0};
    if (!gemm_shape_ok(h)) {                        // launch_gemm would refuse it: never describe a launch that cannot happen
        const int n = snprintf(buf, buf_len, "family=unsupported");
        return (n >= 0 && n < buf_len) ? n : -1;
    }
    const GemmPlan p = gemm_plan(h, gemm_knobs());
    const int n = snprintf(buf, buf_len, "family=%s splits=%d per=%d full=%d tail=%d ex=%d bm=%d group=%d sched=%d ring=%d pipe=%d reduce=%s",
                           gemm_family_name(p.family), p.splits, p.per, p.n_full, p.n_tail, p.ex, p.bm, p.group, p.sched, p.ring, p.pipe, gemm_reduce_name(p.reduce));
    return (n >= 0 && n < buf_len) ? n : -1;
}

// the register-staged kernels of this file
template <int EPI, bool OUT_F32>
static int launch_reg_t(const GemmArgs& a, int family, hipStream_t s) {
    if (family == GF_REG_256x128) return launch_cfg<EPI, OUT_F32, 4, 4>(a, s);
    if constexpr (EPI != EPI_GATEUP) {
        if (family == GF_REG_128x64) return launch_cfg<EPI, OUT_F32, 2, 2>(a, s);
    }
    return launch_cfg<EPI, OUT_F32, 2, 4>(a, s);
}
static int launch_reg(const GemmArgs& a, int family, hipStream_t s) {
    if (a.epi == EPI_GATEUP) return launch_reg_t<EPI_GATEUP, false>(a, family, s);
    if (a.out_f32) return launch_reg_t<EPI_NONE, true>(a, family, s);
    switch (a.epi) {
        case EPI_NONE: return launch_reg_t<EPI_NONE, false>(a, family, s);
        case EPI_GELU_TANH: return launch_reg_t<EPI_GELU_TANH, false>(a, family, s);
        case EPI_GELU_ERF: return launch_reg_t<EPI_GELU_ERF, false>(a, family, s);
    }
    VILA_FAIL(-1, "gemm: unknown epilogue %d", a.epi);
}

int launch_gemm(const GemmArgs& a, hipStream_t s) {
    VILA_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
    if (a.a_cm || a.b_cm) {
        VILA_REQUIRE(a.epi == EPI_NONE && !a.out_f32 && a.W2 == nullptr, "gemm: contraction-major operands take the plain bf16 epilogue only");
        VILA_REQUIRE(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.W % 16 == 0) && ((uintptr_t)a.C % 16 == 0) && a.lda % 8 == 0 && a.ldw % 8 == 0 &&
                     a.ldc % 4 == 0 && a.N % 4 == 0, "gemm: pointers / leading dims must keep 16-B row alignment");
        VILA_REQUIRE(a.residual == nullptr || (a.ldr % 4 == 0 && (uintptr_t)a.residual % 8 == 0), "gemm: residual alignment");
        VILA_REQUIRE(gemm256_supported(a), "gemm: contraction-major operand needs rows %% 8 == 0, K >= 128 (M=%d N=%d K=%d a_cm=%d b_cm=%d)",
                     a.M, a.N, a.K, a.a_cm, a.b_cm);
    } else {
        VILA_REQUIRE(a.K % 8 == 0 && a.N % 4 == 0, "gemm: K (%d) must be a multiple of 8 and N (%d) of 4", a.K, a.N);
        VILA_REQUIRE(a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldc % 4 == 0, "gemm: leading dims must keep 16-B row alignment");
        VILA_REQUIRE(((uintptr_t)a.A % 16 == 0) && ((uintptr_t)a.W % 16 == 0) && ((uintptr_t)a.C % 16 == 0), "gemm: pointers must be 16-B aligned");
        VILA_REQUIRE(a.residual == nullptr || (a.ldr % 4 == 0 && (uintptr_t)a.residual % 8 == 0), "gemm: residual alignment");
        if (a.epi == EPI_GATEUP) {
            VILA_REQUIRE(a.W2 != nullptr && !a.out_f32 && a.bias == nullptr, "gemm: gate/up mode needs W2, bf16 out, no bias");
            VILA_REQUIRE((uintptr_t)a.W2 % 16 == 0, "gemm: W2 alignment");
        } else if (a.out_f32) {
            VILA_REQUIRE(a.epi == EPI_NONE, "gemm: fp32 output only with EPI_NONE");
        }
        if (a.epi < EPI_NONE || a.epi > EPI_GATEUP) VILA_FAIL(-1, "gemm: unknown epilogue %d", a.epi);
    }
    const GemmPlan p = gemm_plan(shape_of(a), gemm_knobs());
    switch (p.family) {
        case GF_256: case GF_256_HYBRID: case GF_CM: case GF_CM_HYBRID: return launch_gemm256(a, p, s);
        case GF_256_SLICED: case GF_CM_SLICED: return launch_gemm256_splitk(a, p, s);
        case GF_RING: return launch_gemm_ring(a, p.ring, p.pipe, s);
        case GF_RING_SPLITK: return launch_gemm_ring_splitk(a, p.splits, s);
        default: return launch_reg(a, p.family, s);
    }
}

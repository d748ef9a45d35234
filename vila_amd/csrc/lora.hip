// The three skinny matrix products of a rank-r (LoRA) adapter, bf16 in, fp32 accumulate, one rounding to bf16 (gfx950, wave64).
//   down :  T[M, R] = scale * X[M, K] . A[R, K]^T                     (t = h A^T;  dt = s dy (B^T)^T)
//   up   :  Y[M, N] = Res[M, N] + scale * T[M, R] . Bt[R, N]          (the adapter's contribution, handed to the base GEMM as its residual)
//   wgrad:  G[R, C] (+)= scale * L[M, R]^T . X[M, C]                  (dBt = s t^T dy;  dA = dt^T x)
// R is the skinny width, a multiple of 16 from 16 to 192 (q|k|v stacked at r = 64).  None of the project's GEMMs serves these: their tiles are
// 256 x 256 or 128 x 64, and an output or a contraction 16-192 wide wastes most of one.
//
// All three use mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15] (j = 0..7), and
// D[row 4 (l >> 4) + reg][col l & 15].
//
// Same bits on every run: no atomics.  `down` splits K and `wgrad` splits M over blocks when the grid would otherwise leave most CUs idle; the
// slices write fp32 partials into the caller's workspace and lora_reduce_kernel adds them in slice order (colsum's scheme, train.hip).
#include "../../include/vila_hip.h"
#include "kernels.h"
#include <algorithm>

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4v;
typedef __attribute__((address_space(3))) bf16x4v lds_bf16x4;

#define LORA_MAX_R 192

__device__ __forceinline__ u32x4 ld16(const bf16_t* p) { return *(const u32x4*)p; }
__device__ __forceinline__ u32x4 zero16() { u32x4 z = {0u, 0u, 0u, 0u}; return z; }
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- down -----------------------------------------------------------------------------------------------------------------------------------
// A block is 32 rows of X (two MFMA row tiles) against all R rows of A over the K slice [blockIdx.y * kper, + kper).  Both operands lie with K
// contiguous, so the fragments come straight from global memory: per 128-wide k chunk and MFMA step s, lane (row, g) reads the 16 bytes
// k = chunk + 32 s + 8 g + j of its row, so the four lanes of a row cover 64 contiguous bytes per load instruction; the A fragment uses the same map.
// The block's four waves deal the slice's chunks among themselves (wave w takes chunks w, w + 4, ...: four times the loads in flight per block at
// the same L2 traffic for A, which every block re-reads: R x K, at most 1.4 MB at the 8B shapes) and add their accumulators through LDS in the
// fixed order ((w3 + w2) + w1) + w0.  X is read once.
template <int NT>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ A, bf16_t* __restrict__ T,
                                                        float* __restrict__ part, int M, int K, int R, int64_t ldx, int64_t lda, int64_t ldt,
                                                        int kper, float scale) {
    __shared__ f32x4 red[2 * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 32;
    const int k0 = blockIdx.y * kper, k1 = min(K, k0 + kper);
    f32x4 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool rowok[2] = {m0 + r < M, m0 + 16 + r < M};
    const bf16_t* xp[2] = {X + (int64_t)min(m0 + r, M - 1) * ldx, X + (int64_t)min(m0 + 16 + r, M - 1) * ldx};
    for (int kb = k0 + 128 * wave; kb < k1; kb += 512) {
        const int kk = kb + 8 * g;
        u32x4 xa[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 4; ++s) xa[i][s] = (rowok[i] && kk + 32 * s < k1) ? ld16(xp[i] + kk + 32 * s) : zero16();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = 16 * t + r;
            const bf16_t* ap = A + (int64_t)min(n, R - 1) * lda + kk;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const u32x4 b = (n < R && kk + 32 * s < k1) ? ld16(ap + 32 * s) : zero16();
                acc[0][t] = mfma16(xa[0][s], b, acc[0][t]);
                acc[1][t] = mfma16(xa[1][s], b, acc[1][t]);
            }
        }
    }
#pragma unroll
    for (int w = 3; w >= 0; --w) {                                        // (block-uniform trip count: every wave meets every barrier)
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    f32x4* slot = &red[(i * NT + t) * 64 + lane];
                    if (w < 3) { const f32x4 o = *slot; acc[i][t][0] += o[0]; acc[i][t][1] += o[1]; acc[i][t][2] += o[2]; acc[i][t][3] += o[3]; }
                    if (w > 0) *slot = acc[i][t];
                }
        }
        if (w > 0) __syncthreads();
    }
    if (wave != 0) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = m0 + 16 * i + 4 * g + j, n = 16 * t + r;
                if (m < M && n < R) {
                    if (part) part[((int64_t)blockIdx.y * M + m) * R + n] = acc[i][t][j];
                    else T[(int64_t)m * ldt + n] = f2bf(scale * acc[i][t][j]);
                }
            }
}

// out[row][col] = bf16(scale * (part[0] + part[1] + ... in slice order) (+ out[row][col])), four columns per thread (cols % 4 == 0)
__global__ __launch_bounds__(256) void lora_reduce_kernel(const float* __restrict__ part, int nslices, int64_t slice_stride, bf16_t* __restrict__ out,
                                                          int rows, int cols, int64_t ld, float scale, int accumulate) {
    const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (idx >= (int64_t)rows * cols) return;
    const int row = (int)(idx / cols), col = (int)(idx % cols);
    f32x4 s = *(const f32x4*)(part + idx);
    for (int i = 1; i < nslices; ++i) {
        const f32x4 p = *(const f32x4*)(part + i * slice_stride + idx);
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += p[3];
    }
    bf16_t* o = out + (int64_t)row * ld + col;
    float v[4] = {scale * s[0], scale * s[1], scale * s[2], scale * s[3]};
    if (accumulate) {
        const u32x2 old = *(const u32x2*)o;
        v[0] += lo_bf(old[0]); v[1] += hi_bf(old[0]); v[2] += lo_bf(old[1]); v[3] += hi_bf(old[1]);
    }
    u32x2 w; w[0] = pack2bf(v[0], v[1]); w[1] = pack2bf(v[2], v[3]);
    *(u32x2*)o = w;
}

// ---- up -------------------------------------------------------------------------------------------------------------------------------------
// A pure streaming kernel: M x N written (and Res read), the contraction is one to six MFMA steps.  The product is computed transposed,
// D[n][m] = sum_k Bt[k][n] T[m][k]: a lane's four accumulator registers are then four consecutive columns of one output row, and with the
// block's 64 columns dealt to (MFMA tile t, tile row i) as column 16 (i >> 2) + 4 t + (i & 3) a lane ends up with 16 consecutive columns
// (two 16-byte stores) and the wave's four lane groups with 128 contiguous bytes of each of its 16 rows.  The Bt fragments (a strided gather,
// once per wave) stay in registers while the wave walks down its rows; the T fragments are 16-byte row reads.
template <int KS>
__global__ __launch_bounds__(256) void lora_up_kernel(const bf16_t* __restrict__ T, const bf16_t* __restrict__ Bt, const bf16_t* __restrict__ Res,
                                                      bf16_t* __restrict__ Y, int M, int N, int R, int64_t ldt, int64_t ldb, int64_t ldres,
                                                      int64_t ldy, int rows_per_block, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 64;
    u32x4 bfrag[4][KS];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * (i >> 2) + 4 * t + (i & 3);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int k = 32 * s + 8 * g + j;
                const uint32_t lo = (n < N && k < R) ? Bt[(int64_t)k * ldb + n] : 0u;
                const uint32_t hi = (n < N && k + 1 < R) ? Bt[(int64_t)(k + 1) * ldb + n] : 0u;
                w[j >> 1] = lo | (hi << 16);
            }
            bfrag[t][s] = u32x4{w[0], w[1], w[2], w[3]};
        }
    }
    const int mbeg = blockIdx.y * rows_per_block, mend = min(M, mbeg + rows_per_block);
    for (int mt = mbeg + 16 * wave; mt < mend; mt += 64) {
        const int m = mt + i;
        const bool mok = m < mend;
        const bf16_t* tp = T + (int64_t)min(m, M - 1) * ldt + 8 * g;
        u32x4 tf[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) tf[s] = (mok && 32 * s + 8 * g < R) ? ld16(tp + 32 * s) : zero16();
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) acc[t] = mfma16(bfrag[t][s], tf[s], acc[t]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = n0 + 16 * g + 8 * h;
            if (mok && c < N) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { v[j] = scale * acc[2 * h][j]; v[4 + j] = scale * acc[2 * h + 1][j]; }
                if (Res) {
                    const u32x4 rr = ld16(Res + (int64_t)m * ldres + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[2 * j] += lo_bf(rr[j]); v[2 * j + 1] += hi_bf(rr[j]); }
                }
                u32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = pack2bf(v[2 * j], v[2 * j + 1]);
                *(u32x4*)(Y + (int64_t)m * ldy + c) = o;
            }
        }
    }
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------------------------
// The contraction runs over the rows, and both operands are read as they lie: 64 rows of L (all R columns) and of X (the block's 64 columns) are
// staged row-major into LDS with 16-byte loads, and both MFMA operands come out of those images through the transposing LDS read
// (ds_read_b64_tr_b16: per 16-lane group a block of 4 rows x 16 columns, lane 4 q + p supplies the address of row q, columns 4 p .. 4 p + 3, and
// lane i receives column i).  Rows past the slice and columns past R / C are staged as zeros, never masked: the transposing read needs every
// lane active and every address inside the image.  Every address is a multiple of 8 bytes (row strides 144 and 32 NT + 16, columns in fours).
// Wave w owns columns 16 w .. 16 w + 15 of the block's 64 and all R rows of G.  The next 64 rows are loaded into registers while this stage is
// multiplied.  blockIdx.y is the M slice [blockIdx.y * mper, + mper), mper a multiple of 64.
template <int NT>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const bf16_t* __restrict__ L, const bf16_t* __restrict__ X, bf16_t* __restrict__ G,
                                                         float* __restrict__ part, int M, int R, int C, int64_t ldl, int64_t ldx, int64_t ldg,
                                                         int mper, float scale, int accumulate) {
    constexpr int MB = 64, XS = 64 * 2 + 16, LS = 32 * NT + 16;
    constexpr int LCH = 2 * NT, LN = (MB * LCH + 255) / 256;             // 16-byte chunks per L row; chunks per thread
    __shared__ __attribute__((aligned(16))) char lds[MB * XS + MB * LS];
    char* const ximg = lds;
    char* const limg = lds + MB * XS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int c0 = blockIdx.x * 64;
    const int mbeg = blockIdx.y * mper, mend = min(M, mbeg + mper);
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 xreg[2], lreg[LN];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ch = tid + 256 * u, row = m0 + (ch >> 3), col = c0 + 8 * (ch & 7);
            xreg[u] = (row < mend && col < C) ? ld16(X + (int64_t)row * ldx + col) : zero16();
        }
#pragma unroll
        for (int u = 0; u < LN; ++u) {
            const int ch = tid + 256 * u, row = m0 + ch / LCH, col = 8 * (ch % LCH);
            lreg[u] = (ch < MB * LCH && row < mend && col < R) ? ld16(L + (int64_t)row * ldl + col) : zero16();
        }
    };
    fetch(mbeg);
    for (int m0 = mbeg; m0 < mend; m0 += MB) {
        __syncthreads();                                                  // the previous stage has been read
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ch = tid + 256 * u;
            *(u32x4*)(ximg + (ch >> 3) * XS + 16 * (ch & 7)) = xreg[u];
        }
#pragma unroll
        for (int u = 0; u < LN; ++u) {
            const int ch = tid + 256 * u;
            if (ch < MB * LCH) *(u32x4*)(limg + (ch / LCH) * LS + 16 * (ch % LCH)) = lreg[u];
        }
        __syncthreads();
        if (m0 + MB < mend) fetch(m0 + MB);                               // (block-uniform; the reads below run with every lane active)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int row = 32 * ks + 8 * grp + q;
            const char* xa = ximg + row * XS + 32 * wave + 8 * p;
            const bf16x4v xlo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)xa);
            const bf16x4v xhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(xa + 4 * XS));
            const bf16x8 xb = __builtin_shufflevector(xlo, xhi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const char* la = limg + row * LS + 32 * t + 8 * p;
                const bf16x4v llo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)la);
                const bf16x4v lhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(la + 4 * LS));
                const bf16x8 lf = __builtin_shufflevector(llo, lhi, 0, 1, 2, 3, 4, 5, 6, 7);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lf, xb, acc[t], 0, 0, 0);
            }
        }
    }
    const int c = c0 + 16 * wave + (lane & 15);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * t + 4 * grp + j;
            if (r < R && c < C) {
                if (part) part[((int64_t)blockIdx.y * R + r) * C + c] = acc[t][j];
                else {
                    bf16_t* o = G + (int64_t)r * ldg + c;
                    float v = scale * acc[t][j];
                    if (accumulate) v += bf2f(*o);
                    *o = f2bf(v);
                }
            }
        }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
struct Split { int n; int per; };

// K slices of `down`: none below K = 1024 or once the rows alone give 256 blocks; 4 below K = 4096, 8 from there; whole 128-wide chunks
Split down_split(int M, int K) {
    const int want = (K < 1024 || cdiv(M, 32) >= 256) ? 1 : (K < 4096 ? 4 : 8);
    const int per = (int)align_up((size_t)cdiv(K, want), 128);
    return {cdiv(K, per), per};
}
// M slices of `wgrad`: none up to 256 rows; above, enough for about 512 blocks, at most 32, whole 64-row stages
Split wgrad_split(int M, int C) {
    if (M <= 256) return {1, (int)align_up((size_t)M, 64)};
    const int want = std::min(32, cdiv(512, cdiv(C, 64)));
    const int per = (int)align_up((size_t)cdiv(M, want), 64);
    return {cdiv(M, per), per};
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int nt_bucket(int R) { const int nt = R / 16; return nt <= 4 ? nt : nt <= 6 ? 6 : nt <= 8 ? 8 : nt <= 9 ? 9 : 12; }

#define LORA_CHECK_R(name) VILA_REQUIRE(R >= 16 && R <= LORA_MAX_R && R % 16 == 0, name ": R = %d must be a multiple of 16 from 16 to %d", R, LORA_MAX_R)
#define LORA_NT_SWITCH(R, CALL) switch (nt_bucket(R)) { case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; \
    case 4: CALL(4); break; case 6: CALL(6); break; case 8: CALL(8); break; case 9: CALL(9); break; default: CALL(12); break; }

int launch_reduce(const float* part, int n, int64_t stride, bf16_t* out, int rows, int cols, int64_t ld, float scale, int accumulate, hipStream_t s) {
    const int64_t quads = (int64_t)rows * cols / 4;
    hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, part, n, stride, out, rows, cols, ld, scale, accumulate);
    VILA_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" size_t vila_lora_down_workspace_bytes(int M, int K, int R) {
    if (M < 1 || K < 1 || R < 1) return 0;
    const Split sp = down_split(M, K);
    return sp.n > 1 ? (size_t)sp.n * M * R * sizeof(float) : 0;
}
extern "C" size_t vila_lora_up_workspace_bytes(int M, int N, int R) { (void)M; (void)N; (void)R; return 0; }
extern "C" size_t vila_lora_wgrad_workspace_bytes(int M, int R, int C) {
    if (M < 1 || C < 1 || R < 1) return 0;
    const Split sp = wgrad_split(M, C);
    return sp.n > 1 ? (size_t)sp.n * R * C * sizeof(float) : 0;
}

extern "C" int vila_lora_down_bf16(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int M, int K, int R, float scale,
                                   void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    LORA_CHECK_R("lora_down");
    VILA_REQUIRE(M >= 1 && K >= 8 && K % 8 == 0, "lora_down: M = %d must be positive and K = %d a positive multiple of 8", M, K);
    VILA_REQUIRE(ldx % 8 == 0 && lda % 8 == 0 && ldt % 8 == 0 && ldx >= K && lda >= K && ldt >= R,
                 "lora_down: every leading dimension must be a multiple of 8 elements and cover its row (ldx %lld, lda %lld, ldt %lld)",
                 (long long)ldx, (long long)lda, (long long)ldt);
    VILA_REQUIRE(X && A && T && al16(X) && al16(A) && al16(T), "lora_down: X, A and T must be 16-byte aligned");
    const Split sp = down_split(M, K);
    const size_t need = vila_lora_down_workspace_bytes(M, K, R);
    VILA_REQUIRE(workspace_bytes >= need && (need == 0 || (workspace && al16(workspace))),
                 "lora_down: workspace of %zu bytes (16-byte aligned) required, %zu given", need, workspace_bytes);
    hipStream_t s = vila_stream_enter((void*)stream);
    float* part = sp.n > 1 ? (float*)workspace : nullptr;
    const dim3 grid(cdiv(M, 32), sp.n);
#define CALL(NT) hipLaunchKernelGGL(lora_down_kernel<NT>, grid, dim3(256), 0, s, (const bf16_t*)X, (const bf16_t*)A, (bf16_t*)T, part, M, K, R, ldx, lda, \
                                    ldt, sp.per, scale)
    LORA_NT_SWITCH(R, CALL)
#undef CALL
    VILA_LAUNCH_CHECK();
    if (part) return launch_reduce(part, sp.n, (int64_t)M * R, (bf16_t*)T, M, R, ldt, scale, 0, s);
    return 0;
}

extern "C" int vila_lora_up_bf16(const void* T, int64_t ldt, const void* Bt, int64_t ldb, const void* Res, int64_t ldres, void* Y, int64_t ldy, int M,
                                 int N, int R, float scale, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    LORA_CHECK_R("lora_up");
    VILA_REQUIRE(M >= 1 && N >= 8 && N % 8 == 0, "lora_up: M = %d must be positive and N = %d a positive multiple of 8", M, N);
    VILA_REQUIRE(ldt % 8 == 0 && ldb % 8 == 0 && ldy % 8 == 0 && ldt >= R && ldb >= N && ldy >= N && (!Res || (ldres % 8 == 0 && ldres >= N)),
                 "lora_up: every leading dimension must be a multiple of 8 elements and cover its row (ldt %lld, ldb %lld, ldres %lld, ldy %lld)",
                 (long long)ldt, (long long)ldb, (long long)ldres, (long long)ldy);
    VILA_REQUIRE(T && Bt && Y && al16(T) && al16(Bt) && al16(Y) && al16(Res), "lora_up: T, Bt, Res and Y must be 16-byte aligned");
    hipStream_t s = vila_stream_enter((void*)stream);
    // rows per block: whole 64-row rounds of the block's four waves, about 1024 blocks in all, so that a wave's Bt gather serves several row tiles
    const int strips = cdiv(N, 64);
    const int rpb = (int)align_up((size_t)std::max(64, cdiv(M, std::max(1, 1024 / strips))), 64);
    const dim3 grid(strips, cdiv(M, rpb));
#define CALL(KS) hipLaunchKernelGGL(lora_up_kernel<KS>, grid, dim3(256), 0, s, (const bf16_t*)T, (const bf16_t*)Bt, (const bf16_t*)Res, (bf16_t*)Y, M, N, R, \
                                    ldt, ldb, ldres, ldy, rpb, scale)
    switch (cdiv(R, 32)) { case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break;
                           default: CALL(6); break; }
#undef CALL
    VILA_LAUNCH_CHECK();
    return 0;
}

extern "C" int vila_lora_wgrad_bf16(const void* L, int64_t ldl, const void* X, int64_t ldx, void* G, int64_t ldg, int M, int R, int C, float scale,
                                    int accumulate, void* workspace, size_t workspace_bytes, vila_stream_t stream) {
    LORA_CHECK_R("lora_wgrad");
    VILA_REQUIRE(M >= 1 && C >= 8 && C % 8 == 0, "lora_wgrad: M = %d must be positive and C = %d a positive multiple of 8", M, C);
    VILA_REQUIRE(ldl % 8 == 0 && ldx % 8 == 0 && ldg % 8 == 0 && ldl >= R && ldx >= C && ldg >= C,
                 "lora_wgrad: every leading dimension must be a multiple of 8 elements and cover its row (ldl %lld, ldx %lld, ldg %lld)",
                 (long long)ldl, (long long)ldx, (long long)ldg);
    VILA_REQUIRE(L && X && G && al16(L) && al16(X) && al16(G), "lora_wgrad: L, X and G must be 16-byte aligned");
    const Split sp = wgrad_split(M, C);
    const size_t need = vila_lora_wgrad_workspace_bytes(M, R, C);
    VILA_REQUIRE(workspace_bytes >= need && (need == 0 || (workspace && al16(workspace))),
                 "lora_wgrad: workspace of %zu bytes (16-byte aligned) required, %zu given", need, workspace_bytes);
    hipStream_t s = vila_stream_enter((void*)stream);
    float* part = sp.n > 1 ? (float*)workspace : nullptr;
    const dim3 grid(cdiv(C, 64), sp.n);
#define CALL(NT) hipLaunchKernelGGL(lora_wgrad_kernel<NT>, grid, dim3(256), 0, s, (const bf16_t*)L, (const bf16_t*)X, (bf16_t*)G, part, M, R, C, ldl, ldx, \
                                    ldg, sp.per, scale, accumulate)
    LORA_NT_SWITCH(R, CALL)
#undef CALL
    VILA_LAUNCH_CHECK();
    if (part) return launch_reduce(part, sp.n, (int64_t)R * C, (bf16_t*)G, R, C, ldg, scale, accumulate, s);
    return 0;
}

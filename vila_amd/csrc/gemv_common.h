// Shared pieces of the decode GEMV kernels (gemv.hip: bf16 weights, gemv_w4.hip: int4 group-quantised weights).
#pragma once
#include "kernels.h"

// ---- CU-balanced row-group map (round 6) -------------------------------------------------------------------------------------------
// The grid-stride walk of rounds 1-5 (group = block * 4 + wave, += grid * 4) balances WAVES, not CUs: blocks b and b + 256 share a CU under
// round-robin dispatch, so with 448 working blocks of a 512-block grid 192 CUs streamed 8 row pairs of down_proj and 64 CUs 4, and 64 CUs took
// 40 of gate/up's groups against 36 on the others — the kernel ends when the fullest CU does.  Here a CU owns groups {j * ncu + cu}: every
// shape of NVILA-8B divides evenly (37 / 7 / 9 / 297 groups per CU), and the waves of the CU's blocks deal its groups among themselves.
// On top, `skew` groups per CU move from the odd XCDs' CUs to the even ones' (the round-6 trace: blocks with an odd (block % 8) stream ~7 %
// slower): every CU takes cf = n / ncu - skew groups by the interleaved map, the rest goes to the even CUs only.
struct CuMap {
    int ncu, cf, n_fast, rem;
    __device__ __forceinline__ CuMap(int n_groups, int ncu_, int skew) {
        ncu = ncu_; n_fast = ncu_ >> 1;
        const bool can = (ncu_ & 7) == 0;
        cf = n_groups / ncu_ - (can ? skew : 0); cf = cf < 0 ? 0 : cf;
        rem = n_groups - cf * ncu_;
        if (!can) { cf = 0x3fffffff; rem = 0; }          // odd grids: the plain interleaved map (count() below handles the bound)
        n_total = n_groups;
    }
    int n_total;
    __device__ __forceinline__ int rank(int cu) const { return (cu >> 3) * 4 + ((cu & 7) >> 1); }
    __device__ __forceinline__ int count(int cu) const {
        if (cf == 0x3fffffff) return n_total > cu ? (n_total - cu + ncu - 1) / ncu : 0;
        const bool fast = (cu & 1) == 0;
        const int r = rank(cu);
        return cf + ((fast && rem > r) ? (rem - r + n_fast - 1) / n_fast : 0);
    }
    __device__ __forceinline__ int gid(int cu, int j) const {
        if (cf == 0x3fffffff || j < cf) return j * ncu + cu;
        return cf * ncu + (j - cf) * n_fast + rank(cu);
    }
};

// ---- greedy pick ---------------------------------------------------------------------------------
// (value, index) merge of the argmax kernels (elementwise.hip): the higher value wins, equal values go to the lower index; a NaN never wins.
// Start from (-inf, 0x7fffffff): rows of -inf alone give their lowest index, rows of NaN alone leave the start pair.
__device__ __forceinline__ void amax_merge(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__device__ __forceinline__ void wave_amax(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64); const int i2 = __shfl_xor(i, o, 64);
        amax_merge(v, i, v2, i2);
    }
}

// ---- activation staging -------------------------------------------------------------------------
// stage x (optionally RMS-normalised with gain, HF rounding order) as bf16 into LDS, once per block of NT threads (NT = 256 x the blocks a CU
// used to hold: one copy per CU instead of one per 256 threads).
// The sum of squares is formed by the FIRST FOUR waves alone, each thread over the chunks tid + 256 i in that order, then wave_sum, then
// scratch[0] + ... + scratch[3]: the summation order of the 256-thread form, so the result does not depend on NT.  The other waves fetch their
// share of x and of the gain meanwhile and join in the scaling and the LDS writes, which are element-wise.
// Single pass for K <= 8192 (x kept in registers between the sum of squares and the scaling).
template <int NT = 256>
__device__ __forceinline__ void stage_x(const bf16_t* x, const bf16_t* __restrict__ norm_w, float eps, int K,
                                        bf16_t* sx, float* scratch) {
    static_assert(NT % 256 == 0 && NT >= 256 && NT <= 1024, "stage_x: 4..16 waves");
    const int tid = threadIdx.x, nch = K >> 3;
    if (norm_w == nullptr) {
        // 4 independent 16-B loads in flight per thread and pass (K = 18944: 3 passes of 256 threads instead of 10 dependent round trips)
        for (int c0 = tid; c0 < nch; c0 += NT * 4) {
            u32x4 t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int c = c0 + NT * i; t[i] = (c < nch) ? *(const u32x4*)(x + c * 8) : (u32x4){0u, 0u, 0u, 0u}; }
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int c = c0 + NT * i; if (c < nch) *(u32x4*)(sx + c * 8) = t[i]; }
        }
        __syncthreads();
        return;
    }
    constexpr int MAXC = 4;                 // chunks per thread of the four summing waves
    constexpr int SC = (256 * MAXC + NT - 1) / NT;   // chunks per thread in the scaling of the single-pass form
    const bool small = nch <= 256 * MAXC;
    u32x4 v[MAXC], xs[SC], gs[SC];
    float s = 0.f;
    if (tid < 256) {
        if (small) {
#pragma unroll
            for (int i = 0; i < MAXC; ++i) {
                const int c = tid + 256 * i;
                v[i] = (c < nch) ? *(const u32x4*)(x + c * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float a = lo_bf(v[i][k]), b = hi_bf(v[i][k]); s += a * a + b * b; }
            }
        } else {
            for (int c = tid; c < nch; c += 256) {
                const u32x4 t = *(const u32x4*)(x + c * 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float a = lo_bf(t[k]), b = hi_bf(t[k]); s += a * a + b * b; }
            }
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) scratch[tid >> 6] = s;
    }
    if constexpr (NT == 256) {
#pragma unroll
        for (int i = 0; i < SC; ++i) xs[i] = v[i];
    } else if (small) {                    // every wave's share of x and of the gain, requested before the wait
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            const int c = tid + NT * i;
            xs[i] = (c < nch) ? *(const u32x4*)(x + c * 8) : (u32x4){0u, 0u, 0u, 0u};
            gs[i] = (c < nch) ? *(const u32x4*)(norm_w + c * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();
    const float rstd = rsqrtf((scratch[0] + scratch[1] + scratch[2] + scratch[3]) / K + eps);
    if (small) {
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            const int c = tid + NT * i;
            if (c < nch) {
                if constexpr (NT == 256) gs[i] = *(const u32x4*)(norm_w + c * 8);
                u32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    o[k] = pack2bf(lo_bf(gs[i][k]) * bfround(lo_bf(xs[i][k]) * rstd), hi_bf(gs[i][k]) * bfround(hi_bf(xs[i][k]) * rstd));
                *(u32x4*)(sx + c * 8) = o;
            }
        }
    } else {
        for (int c = tid; c < nch; c += NT) {
            const u32x4 t = *(const u32x4*)(x + c * 8);
            const u32x4 g = *(const u32x4*)(norm_w + c * 8);
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = pack2bf(lo_bf(g[k]) * bfround(lo_bf(t[k]) * rstd), hi_bf(g[k]) * bfround(hi_bf(t[k]) * rstd));
            *(u32x4*)(sx + c * 8) = o;
        }
    }
    __syncthreads();
}

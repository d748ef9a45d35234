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

// ---- wave reduction without LDS -------------------------------------------------------------------
// The xor butterfly of wave_sum (common.h: v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1, the same partner at every step, so the same bits) on
// the VALU alone.  __shfl_xor is ds_bpermute_b32: six dependent trips over the LDS crossbar, each behind an lgkmcnt wait, at the tail of every
// row group.  Here: lane ^ 32 and ^ 16 by gfx950's row swaps (attn_common.h xor32_max), ^ 8 by a DPP rotation of the 16-lane row, ^ 4 by two
// bank-masked rotations (a DPP lane reads lane (i - n) mod 16 under row_ror:n: the lanes with bit 2 set — banks 1 and 3 — find i ^ 4 = i - 4
// under row_ror:4, the others i + 4 under row_ror:12), ^ 2 and ^ 1 by quad permutations.  IEEE addition is commutative, so which of the two
// swapped values is "this lane's" does not matter (NaN payloads aside).
template <int CTRL, int BANKS = 0xf>
__device__ __forceinline__ float dpp_mov(float old, float x) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(old), __float_as_uint(x), CTRL, 0xf, BANKS, false));
}
__device__ __forceinline__ float wave_sum_xor(float v) {
    unsigned u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    u = __float_as_uint(v);
    r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    v += dpp_mov<0x128>(v, v);                                   // row_ror:8
    v += dpp_mov<0x12c, 0x5>(dpp_mov<0x124, 0xa>(v, v), v);      // row_ror:4 on banks 1, 3; row_ror:12 on banks 0, 2
    v += dpp_mov<0x4e>(v, v);                                    // quad_perm:[2,3,0,1]
    v += dpp_mov<0xb1>(v, v);                                    // quad_perm:[1,0,3,2]
    return v;
}

// ---- activation staging -------------------------------------------------------------------------
// stage x (optionally RMS-normalised with gain, HF rounding order) as bf16 into LDS, once per block of NT threads (NT = 256 x the blocks a CU
// used to hold: one copy per CU instead of one per 256 threads).
// Two halves, so that the caller can put its first weight batch between them (the ordering rule of the batch-1 decode kernels, DESIGN.md §4.3:
// vector loads retire in order per wave, so everything the prologue needs is requested first, the weights behind it, and the prologue waits with
// a counted vmcnt for its own loads alone while the weights are in flight):
//   stage_x_issue  requests into registers, none depending on another and none predicated (a chunk index past the row is clamped to the row's last
//                  chunk and its value dropped in the finish: straight-line code, so the waits count loads instead of draining them): x and the gain of this thread's chunks and, in the four summing waves,
//                  their chunks of the sum of squares; without a norm, the thread's first PC chunks of x;
//   stage_x_finish does the rest: sum of squares, sync, scaling, LDS writes, sync.
// The sum of squares is formed by the FIRST FOUR waves alone, each thread over the chunks tid + 256 i in that order, then wave_sum (or wave_sum_xor: the same bits), then
// scratch[0] + ... + scratch[3]: the summation order of the 256-thread form, so the result does not depend on NT.  The other waves join in the
// scaling and the LDS writes, which are element-wise.
// Single pass for K <= 8192 (x kept in registers between the sum of squares and the scaling); beyond, the first four chunks of the sum of squares
// are requested up front and the rest of both passes follows in the finish.
// The block sync of the staging: it publishes LDS and nothing else.  __syncthreads() is a workgroup fence over every address space, and on gfx950
// the release half of that fence is s_waitcnt vmcnt(0): it would drain the weight batch that the ordering rule keeps in flight across the staging.
__device__ __forceinline__ void sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
template <bool LDS_SYNC>
__device__ __forceinline__ void stage_sync() {
    if constexpr (LDS_SYNC) sync_lds(); else __syncthreads();
}
template <int NT>
struct StageX {
    static_assert(NT % 256 == 0 && NT >= 256 && NT <= 1024, "stage_x: 4..16 waves");
    static constexpr int MAXC = 4;                          // chunks per thread of the four summing waves
    static constexpr int SC = (256 * MAXC + NT - 1) / NT;   // chunks per thread in the scaling of the single-pass form
    static constexpr int PC = MAXC + 1;                     // no norm: chunks per thread requested up front (K = 18944, NT = 512: all of x),
                                                            // held in v[0 .. MAXC - 1] and t
};
// the registers between the two halves (separate arrays: as members of one struct some of them stayed in scratch)
#define STAGE_X_REGS(NT, name) u32x4 name##_v[StageX<NT>::MAXC], name##_xs[StageX<NT>::SC], name##_gs[StageX<NT>::SC], name##_t
#define STAGE_X_ARGS(name) name##_v, name##_xs, name##_gs, name##_t
template <int NT>
__device__ __forceinline__ void stage_x_issue(const bf16_t* x, const bf16_t* __restrict__ norm_w, int K, u32x4 (&v)[StageX<NT>::MAXC],
                                              u32x4 (&xs)[StageX<NT>::SC], u32x4 (&gs)[StageX<NT>::SC], u32x4& t) {
    using S = StageX<NT>;
    const int tid = threadIdx.x, nch = K >> 3, last = nch - 1;
    if (norm_w == nullptr) {
#pragma unroll
        for (int i = 0; i < S::PC; ++i) { const int c = tid + NT * i; (i < S::MAXC ? v[i] : t) = *(const u32x4*)(x + (c < nch ? c : last) * 8); }
        return;
    }
    const bool small = nch <= 256 * S::MAXC;
    if (tid < 256) {
#pragma unroll
        for (int i = 0; i < S::MAXC; ++i) { const int c = tid + 256 * i; v[i] = *(const u32x4*)(x + (c < nch ? c : last) * 8); }
    }
    if (small) {                           // every wave's share of x and of the gain
#pragma unroll
        for (int i = 0; i < S::SC; ++i) {
            const int c = tid + NT * i < nch ? tid + NT * i : last;
            if constexpr (NT != 256) xs[i] = *(const u32x4*)(x + c * 8);
            gs[i] = *(const u32x4*)(norm_w + c * 8);
        }
    }
}
// LDS_SYNC: the block syncs are sync_lds() (callers with loads in flight that the staging must not drain); otherwise __syncthreads()
// XOR_SUM: the sum of squares is reduced by wave_sum_xor (the same bits as wave_sum, no LDS trip in front of the first barrier)
template <int NT, bool LDS_SYNC, bool XOR_SUM = false>
__device__ __forceinline__ void stage_x_finish(const bf16_t* x, const bf16_t* __restrict__ norm_w, float eps, int K, bf16_t* sx, float* scratch,
                                               u32x4 (&v)[StageX<NT>::MAXC], u32x4 (&xs)[StageX<NT>::SC], u32x4 (&gs)[StageX<NT>::SC],
                                               u32x4& t) {
    using S = StageX<NT>;
    const int tid = threadIdx.x, nch = K >> 3;
    if (norm_w == nullptr) {
#pragma unroll
        for (int i = 0; i < S::PC; ++i) { const int c = tid + NT * i; if (c < nch) *(u32x4*)(sx + c * 8) = i < S::MAXC ? v[i] : t; }
        // longer rows: 4 independent 16-B loads in flight per thread and pass
        for (int c0 = tid + NT * S::PC; c0 < nch; c0 += NT * 4) {
            u32x4 r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int c = c0 + NT * i; r[i] = (c < nch) ? *(const u32x4*)(x + c * 8) : (u32x4){0u, 0u, 0u, 0u}; }
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int c = c0 + NT * i; if (c < nch) *(u32x4*)(sx + c * 8) = r[i]; }
        }
        stage_sync<LDS_SYNC>();
        return;
    }
    const bool small = nch <= 256 * S::MAXC;
    if (tid < 256) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < S::MAXC; ++i) {
            const u32x4 vi = (tid + 256 * i < nch) ? v[i] : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float a = lo_bf(vi[k]), b = hi_bf(vi[k]); s += a * a + b * b; }
        }
        if (!small) {
            for (int c = tid + 256 * S::MAXC; c < nch; c += 256) {
                const u32x4 t = *(const u32x4*)(x + c * 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float a = lo_bf(t[k]), b = hi_bf(t[k]); s += a * a + b * b; }
            }
        }
        s = XOR_SUM ? wave_sum_xor(s) : wave_sum(s);
        if ((tid & 63) == 0) scratch[tid >> 6] = s;
    }
    if constexpr (NT == 256) {
#pragma unroll
        for (int i = 0; i < S::SC; ++i) xs[i] = v[i];
    }
    stage_sync<LDS_SYNC>();
    const float rstd = rsqrtf((scratch[0] + scratch[1] + scratch[2] + scratch[3]) / K + eps);
    if (small) {
#pragma unroll
        for (int i = 0; i < S::SC; ++i) {
            const int c = tid + NT * i;
            if (c < nch) {
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
    stage_sync<LDS_SYNC>();
}

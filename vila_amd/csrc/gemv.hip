// Batch-1 decode kernels (HOT LOOP #3): every weight byte is read exactly once per token, so
// the roofline is HBM (14.14 GB / token for NVILA-8B bf16), not MFMA.  Design rules (cdna guide, "GEMV / M<=16"):
// weights go straight HBM -> VGPR with 16-B non-temporal loads, deep unroll, late wait; the activation vector is
// staged once per block in LDS (with the preceding RMSNorm fused in, HF rounding order kept); all epilogues
// (bias, RoPE, KV-cache write, SiLU*up, residual add) are fused so a decoder layer is 5 launches.
// The head of a kernel: what its first memory requests need arrives as flat leading arguments, preloaded into SGPRs at wave start (this file and
// attn_decode.hip are built with the kernarg preload count set, vila_amd/build.py); the CU map is planned on the host (gemv_plan.h); the rest of
// the arguments is a by-value struct fetched behind the first requests.  See gemv_kernel below and DESIGN.md §4.3.
#include "kernels.h"
#include "gemv_common.h"
#include "gemv_plan.h"
#include "attn_decode.h"

__device__ __forceinline__ u32x4 ldg_nt(const bf16_t* p) { return __builtin_nontemporal_load((const u32x4*)p); }

__device__ __forceinline__ float dot8(const u32x4 w, const u32x4 x, float acc) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc = fmaf(lo_bf(w[k]), lo_bf(x[k]), acc);
        acc = fmaf(hi_bf(w[k]), hi_bf(x[k]), acc);
    }
    return acc;
}

// A bf16 epilogue operand that was requested ahead of the dot product, converted where it is used.  The empty asm keeps the compiler from moving
// the conversion up to the load, where it would wait for the load — and, loads retiring in order, for every weight requested in front of it.
__device__ __forceinline__ float bf2f_late(bf16_t raw) {
    unsigned r = raw;
    asm volatile("" : "+v"(r));
    return __uint_as_float(r << 16);
}

// stage x = merged split-KV attention output (flash-decoding combine fused into the o_proj GEMV):
//   o[h][d] = sum_s exp(m_s - M) part_o[s][h][d] / sum_s exp(m_s - M) l_s ,  rounded to bf16 like the reference's attn output
// In two halves like stage_x (gemv_common.h).  The issue half requests, for every slice of the CAPACITY (n_splits <= MERGE_MAXS; the workspace is
// sized for it), the (m, l) pair of this thread's head and this thread's first MERGE_PI chunks of part_o, without waiting for the position.  The
// finish half drops the slices at or past n_active by SELECTION (they hold stale bytes, so never by a zero weight) and merges exactly as
// attn_merge_weights (attn_decode.h) and the slice-ordered fmaf sum always did: M by fmaxf over s = 0 .. n_active - 1 in order, L and the weights
// by the same expressions, one thread per head; the weighted sum by fmaf in slice order, one thread per chunk.
#define MERGE_MAXS 8                     // slices of the capacity (256-key slices of caches up to 2048 positions)
#define MERGE_PI 2                       // float4 chunks per thread requested up front (28 heads, NT = 512: all of them)
struct AttnMergeLoads { float m[MERGE_MAXS], l[MERGE_MAXS]; f32x4 po[MERGE_PI][MERGE_MAXS]; };
template <int NT>
__device__ __forceinline__ void stage_x_attn_issue(const float* __restrict__ part_o, const float* __restrict__ part_ml, int n_splits, int nq,
                                                   AttnMergeLoads& ld) {
    const int tid = threadIdx.x, n4 = nq * 32;   // float4 chunks
    // No load is predicated per lane (an index past the end is clamped to the last slot and its value never used): straight-line code, so the
    // finish waits with a count.  Slices 4 .. 7 sit behind ONE block-uniform branch, so that a cache of up to 1024 positions requests 4.
    auto issue = [&](int s0) {
#pragma unroll
        for (int s = s0; s < s0 + MERGE_MAXS / 2; ++s) {
            const int sc = s < n_splits ? s : n_splits - 1;
            const float* ml = part_ml + ((int64_t)sc * nq + (tid < nq ? tid : nq - 1)) * 2;
            ld.m[s] = ml[0]; ld.l[s] = ml[1];
#pragma unroll
            for (int it = 0; it < MERGE_PI; ++it) {
                const int i = tid + NT * it < n4 ? tid + NT * it : n4 - 1;
                ld.po[it][s] = *(const f32x4*)(part_o + ((int64_t)sc * nq) * 128 + i * 4);
            }
        }
    };
    issue(0);
    if (n_splits > MERGE_MAXS / 2) issue(MERGE_MAXS / 2);
}
template <int NT>
__device__ __forceinline__ void stage_x_attn_finish(const float* __restrict__ part_o, const float* __restrict__ part_ml, int n_active, int nq,
                                                    bf16_t* sx, float* wsm /* [n_splits * nq] */, const AttnMergeLoads& ld) {
    const int tid = threadIdx.x;
    if (tid < nq) {
        float M = -INFINITY;
#pragma unroll
        for (int s = 0; s < MERGE_MAXS; ++s) if (s < n_active) M = fmaxf(M, ld.m[s]);
        float L = 0.f;
#pragma unroll
        for (int s = 0; s < MERGE_MAXS; ++s) if (s < n_active) L += __expf(ld.m[s] - M) * ld.l[s];
        const float invL = 1.f / L;
#pragma unroll
        for (int s = 0; s < MERGE_MAXS; ++s) if (s < n_active) wsm[s * nq + tid] = __expf(ld.m[s] - M) * invL;
    }
    sync_lds();
    const int n4 = nq * 32;
#pragma unroll
    for (int it = 0; it < MERGE_PI; ++it) {
        const int i = tid + NT * it;
        if (i < n4) {
            const int h = i >> 5;
            f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < MERGE_MAXS; ++s) {
                if (s < n_active) {
                    const f32x4 pv = ld.po[it][s];
                    const float w = wsm[s * nq + h];
                    o[0] = fmaf(w, pv[0], o[0]); o[1] = fmaf(w, pv[1], o[1]); o[2] = fmaf(w, pv[2], o[2]); o[3] = fmaf(w, pv[3], o[3]);
                }
            }
            u32x2 r; r[0] = pack2bf(o[0], o[1]); r[1] = pack2bf(o[2], o[3]);
            *(u32x2*)(sx + i * 4) = r;
        }
    }
    for (int i = tid + NT * MERGE_PI; i < n4; i += NT) {          // more heads than the up-front chunks cover (small grids: NT = 256)
        const int h = i >> 5;
        f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < n_active; ++s) {
            const f32x4 pv = *(const f32x4*)(part_o + ((int64_t)s * nq) * 128 + i * 4);
            const float w = wsm[s * nq + h];
            o[0] = fmaf(w, pv[0], o[0]); o[1] = fmaf(w, pv[1], o[1]); o[2] = fmaf(w, pv[2], o[2]); o[3] = fmaf(w, pv[3], o[3]);
        }
        u32x2 r; r[0] = pack2bf(o[0], o[1]); r[1] = pack2bf(o[2], o[3]);
        *(u32x2*)(sx + i * 4) = r;
    }
    sync_lds();
}

// ---- weight streaming -----------------------------------------------------------------------------
template <int R, int U> struct Batch { u32x4 v[U][R]; };

template <int R, int U>
__device__ __forceinline__ void load_batch(const bf16_t* const (&wrow)[R], int c0, int lane, int nch, Batch<R, U>& b) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = c0 + u * 64 + lane;
#pragma unroll
        for (int r = 0; r < R; ++r) b.v[u][r] = (c < nch) ? ldg_nt(wrow[r] + c * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
}
// A wave's FIRST batch, requested between the two halves of the staging.  Nothing here is predicated or branched over, so that the code from
// the staging's loads to its waits is straight-line and those waits COUNT this batch instead of draining it (behind a join with a path that
// requested fewer loads the compiler's wait falls back to the smaller count): a chunk past the row is clamped to the row's last chunk, and a
// wave without a row group (`has` false; its rows are group 0's) requests the first 16 bytes of those rows in every lane and request — one
// cache line each, so that it stays on the same path at next to no traffic.  first_batch_mask then puts the zeros of load_batch in place of
// the clamped chunks.
template <int R, int U>
__device__ __forceinline__ void load_first_batch(const bf16_t* const (&wrow)[R], int lane, int nch, bool has, Batch<R, U>& b) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = u * 64 + lane < nch ? u * 64 + lane : nch - 1;
#pragma unroll
        for (int r = 0; r < R; ++r) b.v[u][r] = ldg_nt(wrow[r] + (has ? c : 0) * 8);
    }
}
template <int R, int U>
__device__ __forceinline__ void first_batch_mask(int lane, int nch, Batch<R, U>& b) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) b.v[u][r] = (u * 64 + lane < nch) ? b.v[u][r] : (u32x4){0u, 0u, 0u, 0u};
}
template <int R, int U>
__device__ __forceinline__ void fma_batch(const Batch<R, U>& b, const bf16_t* sx, int c0, int lane, int nch, float (&acc)[R]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = c0 + u * 64 + lane;
        const u32x4 xv = (c < nch) ? *(const u32x4*)(sx + c * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = dot8(b.v[u][r], xv, acc[r]);
    }
}
// ---- the tail of a kernel: counted waits inside a batch, a reduction without LDS --------------------------------------
// A wave's loads retire in order, so chunk 0 of a batch can be consumed while chunks 1 .. U - 1 are in flight — if the code from the batch's
// loads to its waits is straight-line (behind a predicated load's join the compiler's wait falls back to a drain) and the dot product takes
// the chunks in the order they were requested.  Mid-kernel the other waves of the SIMD hide the difference; on a wave's last group, which is
// the kernel's tail, and where a wave has one group only (o_proj, down), nothing does.
// A FULL batch (c0 + 64 U <= nch) is requested unpredicated; a partial one clamps every chunk index to the row's last chunk (no new address
// is read) and puts load_batch's zeros in place of the clamped chunks where they are consumed.
// The weights are global memory, and said to be: a flat load counts on both counters and its wait is a drain.  Chunk u's R requests stay in
// front of chunk u + 1's (the scheduler would otherwise go row by row, and the first chunk would wait for half the batch).
__device__ __forceinline__ u32x4 ldg_nt_global(const bf16_t* p) {
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4*)p);
}
template <int R, int U>
__device__ __forceinline__ void load_batch_full(const bf16_t* const (&wrow)[R], int c0, int lane, Batch<R, U>& b) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int r = 0; r < R; ++r) b.v[u][r] = ldg_nt_global(wrow[r] + (c0 + u * 64 + lane) * 8);
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int R, int U>
__device__ __forceinline__ void load_batch_clamped(const bf16_t* const (&wrow)[R], int c0, int lane, int nch, Batch<R, U>& b) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = c0 + u * 64 + lane < nch ? c0 + u * 64 + lane : nch - 1;
#pragma unroll
        for (int r = 0; r < R; ++r) b.v[u][r] = ldg_nt_global(wrow[r] + c * 8);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// Chunk by chunk in request order, the scheduler held to it, so that the wait in front of chunk u leaves the R (U - 1 - u) later loads
// outstanding.  The LDS read of x for chunk u + 1 goes out in front of chunk u's wait (one chunk of arithmetic covers an LDS trip; all U reads
// up front would hold 4 U registers and cost a wave per SIMD).  Per acc[r] the fmaf chain is fma_batch's: u-major, then k.
template <int R, int U, bool FULL>
__device__ __forceinline__ void fma_batch_counted(const Batch<R, U>& b, const bf16_t* sx, int c0, int lane, int nch, float (&acc)[R]) {
    auto read_x = [&](int u) {
        const int c = c0 + u * 64 + lane;
        return *(const u32x4*)(sx + (FULL || c < nch ? c : nch - 1) * 8);
    };
    u32x4 xc = read_x(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        u32x4 xn = xc;
        if (u + 1 < U) xn = read_x(u + 1);
        __builtin_amdgcn_sched_barrier(0);
        const bool in = FULL || c0 + u * 64 + lane < nch;
        const u32x4 x = in ? xc : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = dot8(in ? b.v[u][r] : (u32x4){0u, 0u, 0u, 0u}, x, acc[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[r]));   // chunk u + 1 starts from chunk u's sums: no arithmetic of it moves up (bf2f_late's pin)
        xc = xn;
    }
    __builtin_amdgcn_sched_barrier(0);
}
// a batch already requested (full or clamped, by one wave-uniform choice behind its loads: neither arm requests anything from memory)
template <int R, int U>
__device__ __forceinline__ void fma_batch_any(const Batch<R, U>& b, const bf16_t* sx, int c0, int lane, int nch, float (&acc)[R]) {
    if (c0 + 64 * U <= nch) fma_batch_counted<R, U, true>(b, sx, c0, lane, nch, acc);
    else fma_batch_counted<R, U, false>(b, sx, c0, lane, nch, acc);
}
// dot products of R rows with x (LDS) for chunks [c_start, nch); accumulates into acc, then reduces across the wave.
// CW: counted waits inside a batch (above); XS: wave_sum_xor.  Both keep every bit; which kernels take them is decided per instantiation.
template <int R, int U, bool CW, bool XS>
__device__ __forceinline__ void wave_rows_dot(const bf16_t* const (&wrow)[R], const bf16_t* sx, int K, int lane, float (&acc)[R], int c_start) {
    const int nch = K >> 3;
    if constexpr (CW) {
        int c0 = c_start;
        for (; c0 + 64 * U <= nch; c0 += 64 * U) {
            Batch<R, U> b;
            load_batch_full<R, U>(wrow, c0, lane, b);
            fma_batch_counted<R, U, true>(b, sx, c0, lane, nch, acc);
        }
        if (c0 < nch) {
            Batch<R, U> b;
            load_batch_clamped<R, U>(wrow, c0, lane, nch, b);
            fma_batch_counted<R, U, false>(b, sx, c0, lane, nch, acc);
        }
    } else {
        for (int c0 = c_start; c0 < nch; c0 += 64 * U) {
            Batch<R, U> b;
            load_batch<R, U>(wrow, c0, lane, nch, b);
            fma_batch<R, U>(b, sx, c0, lane, nch, acc);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = XS ? wave_sum_xor(acc[r]) : wave_sum(acc[r]);
}
// Which instantiations take the two parts: decided per kernel from two kernel-trace profiles per build (CHANGELOG), like gemv_flat_head below.
constexpr bool gemv_tail_dpp(int MODE, int U) { return !(MODE == 0 && U == 7); }
constexpr bool gemv_counted_waits(int MODE, int U) { return !(MODE == 0 && U == 7); }
constexpr bool qkv_tail_dpp(int U) { return true; }
constexpr bool qkv_counted_waits(int U) { return true; }

// ------------------------------------------------------------------------------------------------
// generic GEMV: y = W x (+bias) (+residual)   |   gate/up: y = silu(Wg x) * (Wu x)   |   x from attention partials
// Order of the prologue.  A wave's vector loads retire in order.  INPUTS_FIRST: the wave requests (1) every small load the
// staging needs, (2) its first weight batch, and then (3) waits for (1) alone — a counted vmcnt that leaves the weights outstanding — and
// forms the merge, writes LDS and takes the block syncs while the weights are in flight.  That is the merge mode (o_proj) and every plain GEMV
// over rows longer than hidden (U = 4).  Of the latter only down_proj, which has no norm, was measured; with a norm the staging's loads still
// sit behind `tid < 256` and the one- or two-pass choice, so some of its waits may fall back to a smaller count (correct either way).  The
// GEMVs over K = hidden (lm_head, gate/up, and the QKV kernel below) measured no gain and keep the weights in front: their staging then waits
// until the batch has landed.  Figures: DESIGN.md §4.3, CHANGELOG.
// ------------------------------------------------------------------------------------------------
// U = 16-B loads in flight per row and lane: 7 covers a whole K = 3584 row in ONE round trip (the short K=hidden GEMVs are
// latency-bound), 4 is enough for the long rows (K = 18944) where many iterations pipeline anyway.
// NT = threads per block.  On the CU map ONE block of 256 x (blocks per CU of the balanced grid) threads runs per CU, so the activation is
// loaded, normalised and written to LDS once per CU; its NT / 64 waves deal the CU's row groups (j = wave, stride NT / 64).
// Kernel arguments ("the head of a kernel").  What the FIRST memory requests need comes first and flat — four pointers and six
// ints, 14 dwords — so that the wave starts with them in SGPRs (kernarg preload; gemv.hip is built with the preload count set, vila_amd/build.py)
// and requests its first weight batch without a scalar load, a wait or a division in front: the weights, then per mode
//   0: a1 = x, a2 = norm_w          1: a1 = x, a2 = W2, a3 = norm_w          2: a1 = part_o, a2 = part_ml, a3 = pos_ptr,
// K, N, n_splits (mode 2) and the CU map as launch_gemv planned it (gemv_plan.h GemvPlan; ncu_xr == 0: small grids, cf = the walk's stride).
// The head reads neither blockDim nor gridDim (hidden arguments: a scalar load each).  Everything else is GemvTail, a by-value struct behind
// them, fetched right after the first requests (tail_here).
struct GemvTail {
    const bf16_t* bias; const bf16_t* residual; bf16_t* y; float* y_f32; float* amax_v; int* amax_i;
    float eps; int split_keys;
};
// The tail's scalar loads belong HERE: behind the requests already made and in front of everything that follows (left alone the compiler sinks
// them to their first uses, behind the staging's barrier, where each is one more round trip in line).
__device__ __forceinline__ void tail_here(const GemvTail& t) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" :: "s"(t.bias), "s"(t.residual), "s"(t.y), "s"(t.y_f32), "s"(t.amax_v), "s"(t.amax_i), "s"(t.eps), "s"(t.split_keys));
    __builtin_amdgcn_sched_barrier(0);
}
// Which instantiations take the flat head: decided per kernel from two kernel-trace profiles per build (CHANGELOG).  lm_head (<0,7,...>: one
// launch of 172 us per token) measured inside its spread and keeps the head it had: GemvArgs by value, the map derived on the device (CuMap).
constexpr bool gemv_flat_head(int MODE, int U) { return !(MODE == 0 && U == 7); }

// The body both heads share.  Map: GemvPlan (host-planned) or CuMap (device-derived) — the same count() / gid().  FLAT: pin the tail's loads.
template <int MODE, int U, int NT, bool FLAT, class Map>   // MODE 0 plain, 1 gate/up, 2 plain with x = merged attention partials
__device__ __forceinline__ void gemv_body(const bf16_t* W, const void* a1, const void* a2, const void* a3, int K, int N, int n_splits, const Map& cm,
                                          int ncu, int stride, const GemvTail& t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* sx = (bf16_t*)smem;
    float* scratch = (float*)(smem + ((K * 2 + 15) & ~15));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = K >> 3;
    const int n_groups = (N + 1) >> 1;
    constexpr int R = (MODE == 1) ? 4 : 2;
    constexpr bool INPUTS_FIRST = MODE == 2 || (MODE == 0 && U < 7);
    constexpr bool CW = gemv_counted_waits(MODE, U), XS = gemv_tail_dpp(MODE, U);
    const bf16_t* const W2 = (const bf16_t*)a2;                                                   // mode 1
    const bf16_t* const x = (const bf16_t*)a1;                                                    // modes 0, 1
    const bf16_t* const norm_w = (const bf16_t*)(MODE == 1 ? a3 : a2);                            // modes 0, 1
    // ncu > 0: the CU-balanced map (block = CU); ncu == 0: small grids, the plain grid-stride walk (stride = blocks x WPB)
    constexpr int WPB = NT / 64;
    const int cu = ncu > 0 ? (int)blockIdx.x : 0;
    const int cnt = ncu > 0 ? cm.count(cu) : 0;
    int j = wave;                                                             // the block's WPB waves deal the CU's groups
    int g = ncu > 0 ? (j < cnt ? cm.gid(cu, j) : n_groups) : blockIdx.x * WPB + wave;
    auto next_group = [&]() { if (ncu > 0) { j += WPB; g = j < cnt ? cm.gid(cu, j) : n_groups; } else g += stride; };

    auto rows_of = [&](int gg, const bf16_t* (&rows)[R]) {
        if constexpr (CW) gg = __builtin_amdgcn_readfirstlane(gg);   // a group belongs to a wave, and said so its row bases are scalars: fewer address registers
        const int n = gg * 2;
        const int n1 = (n + 1 < N) ? n + 1 : n;
        if constexpr (MODE == 1) {
            rows[0] = W + (int64_t)n * K; rows[1] = W2 + (int64_t)n * K;
            rows[2] = W + (int64_t)n1 * K; rows[3] = W2 + (int64_t)n1 * K;
        } else {
            rows[0] = W + (int64_t)n * K; rows[1] = W + (int64_t)n1 * K;
        }
    };
    // Epilogue: after the wave reduction every lane holds the sums; lanes 0 and 1 each produce and store one of the wave's two adjacent
    // outputs (rows n, n + 1).
    bf16_t e_bias = 0, e_res = 0;                    // as loaded (bf2f_late)
    float best = -INFINITY; int bi = 0x7fffffff;     // t.amax_v: the largest fp32 output of this lane's rows so far (lanes 0 and 1)
    auto finish = [&](int gg, float (&acc)[R]) {
        const int n = gg * 2;
        bf16_t o = 0;
        if constexpr (MODE == 1) {
            // HF: down(act(gate(x)) * up(x)) with every tensor rounded to bf16
            const float gv = bfround(lane == 0 ? acc[0] : acc[2]), uv = bfround(lane == 0 ? acc[1] : acc[3]);
            o = f2bf(bfround(silu_f(gv)) * uv);
        } else {
            float v = lane == 0 ? acc[0] : acc[1];
            v += bf2f_late(e_bias);
            if (lane < 2 && n + lane < N && t.y_f32 != nullptr) t.y_f32[n + lane] = v;
            if (t.amax_v != nullptr && lane < 2 && n + lane < N) amax_merge(best, bi, v, n + lane);
            if (t.residual != nullptr) v = bfround(v) + bf2f_late(e_res);
            o = f2bf(v);
        }
        if (t.y != nullptr && lane < 2 && n + lane < N) t.y[n + lane] = o;
    };
    // the epilogue's operands are requested BEFORE the dot product: fetched after the reduction they add a dependent memory round
    // trip (~1 us) to the tail of every wave, i.e. to the kernel
    auto epi_fetch = [&](int gg) {
        if constexpr (MODE != 1) {
            const int nn = gg * 2 + lane;
            e_bias = 0; e_res = 0;
            if (lane < 2 && nn < N) {
                if (t.bias != nullptr) e_bias = t.bias[nn];
                if (t.residual != nullptr && t.y != nullptr) e_res = t.residual[nn];
            }
        }
    };

    const bf16_t* rows[R];
    Batch<R, U> b0;
    const bool has = g < n_groups;
    if constexpr (INPUTS_FIRST) {
        rows_of(has ? g : 0, rows);
        if constexpr (MODE == 2) {
            const int pos = *(const int32_t*)a3;               // its pointer is here at wave start: requested in front of the tail's wait, not behind it
            __builtin_amdgcn_sched_barrier(0);
            AttnMergeLoads ld;
            stage_x_attn_issue<NT>((const float*)a1, (const float*)a2, n_splits, K >> 7, ld);
            __builtin_amdgcn_sched_barrier(0);                   // the staging's loads stay in front of the weights
            load_first_batch<R, U>(rows, lane, nch, has, b0);
            if constexpr (FLAT) tail_here(t);
            if (has) epi_fetch(g);
            const int ks = t.split_keys > 0 ? t.split_keys : DEC_KS;
            const int n_active = (pos + ks) / ks;                // ceil((pos+1)/ks)
            stage_x_attn_finish<NT>((const float*)a1, (const float*)a2, n_active < n_splits ? n_active : n_splits, K >> 7, sx, scratch, ld);
        } else {
            STAGE_X_REGS(NT, st);
            stage_x_issue<NT>(x, norm_w, K, STAGE_X_ARGS(st));
            __builtin_amdgcn_sched_barrier(0);
            load_first_batch<R, U>(rows, lane, nch, has, b0);
            if constexpr (FLAT) tail_here(t);
            if (has) epi_fetch(g);                               // behind the weights: in front, the staging's loads waited for it at a join
            stage_x_finish<NT, true, XS>(x, norm_w, t.eps, K, sx, scratch, STAGE_X_ARGS(st));
        }
        if constexpr (!CW) { if (has) first_batch_mask<R, U>(lane, nch, b0); }   // CW: masked where consumed (fma_batch_counted)
    } else {
        // the first weight batch in front of the staging, for short rows only (K <= 4096: the staging latency is comparable to the stream)
        if (has && K <= 4096) { rows_of(g, rows); load_batch<R, U>(rows, 0, lane, nch, b0); }
        if constexpr (FLAT) tail_here(t);
        if (has) epi_fetch(g);
        STAGE_X_REGS(NT, st);
        stage_x_issue<NT>(x, norm_w, K, STAGE_X_ARGS(st));
        stage_x_finish<NT, false, XS>(x, norm_w, t.eps, K, sx, scratch, STAGE_X_ARGS(st));   // __syncthreads(): exactly the waits these kernels had
    }
    if (has && (INPUTS_FIRST || K <= 4096)) {
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        if constexpr (CW) fma_batch_any<R, U>(b0, sx, 0, lane, nch, acc); else fma_batch<R, U>(b0, sx, 0, lane, nch, acc);
        wave_rows_dot<R, U, CW, XS>(rows, sx, K, lane, acc, 64 * U);
        finish(g, acc);
        next_group();
    }
    for (; g < n_groups; next_group()) {
        rows_of(g, rows);
        epi_fetch(g);
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        wave_rows_dot<R, U, CW, XS>(rows, sx, K, lane, acc, 0);
        finish(g, acc);
    }
    // the greedy pick's first stage (lm_head of the batch-1 step): this block's rows reduced to one (max, index) pair with argmax's tie rule
    if constexpr (MODE == 0) {
        if (t.amax_v != nullptr) {
            __shared__ float sv[WPB];
            __shared__ int si[WPB];
            wave_amax(best, bi);
            if (lane == 0) { sv[wave] = best; si[wave] = bi; }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int w = 1; w < WPB; ++w) amax_merge(best, bi, sv[w], si[w]);
                t.amax_v[blockIdx.x] = best; t.amax_i[blockIdx.x] = bi;
            }
        }
    }
}

template <int MODE, int U, int NT>
__global__ __launch_bounds__(NT) void gemv_kernel(const bf16_t* W, const void* a1, const void* a2, const void* a3, int K, int N, int n_splits, int ncu_xr,
                                                  int cf, int xq, GemvTail t) {
    const GemvPlan cm{ncu_xr, cf, xq};
    gemv_body<MODE, U, NT, true>(W, a1, a2, a3, K, N, n_splits, cm, cm.ncu(), cf, t);
}
template <int MODE, int U, int NT>
__global__ __launch_bounds__(NT) void gemv_kernel_args(GemvArgs p, int n_groups, int ncu, int skew) {
    const CuMap cm(n_groups, ncu > 0 ? ncu : 8, ncu > 0 ? skew : 0);
    const GemvTail t{p.bias, p.residual, p.y, p.y_f32, p.amax_v, p.amax_i, p.eps, p.split_keys};
    gemv_body<MODE, U, NT, false>(p.W, MODE == 2 ? (const void*)p.part_o : (const void*)p.x,
                                  MODE == 2 ? (const void*)p.part_ml : MODE == 1 ? (const void*)p.W2 : (const void*)p.norm_w,
                                  MODE == 2 ? (const void*)p.pos_ptr : MODE == 1 ? (const void*)p.norm_w : nullptr, p.K, p.N, p.n_splits, cm, ncu, (int)gridDim.x * (NT / 64), t);
}

// Grid sizing for the HBM-bound GEMVs: one block per CU (the dispatcher deals blocks round-robin, so 448 blocks of 256 threads would leave
// 64 CUs with half the work of the others) of up to GEMV_BPC x 256 threads (4 = 16 waves = everything resident at once); the waves of a
// block deal that CU's row groups (CuMap, gemv_common.h).
#define GEMV_BPC 4
static int gemv_cu_count() {
    static thread_local int per_dev[16] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int& n = per_dev[dev & 15];
    if (n == 0) {
        hipDeviceProp_t prop;
        n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return n;
}
// grid of an HBM-bound GEMV: one block of 256 x *per_out (1..4) threads per CU (*ncu_out = CUs) whose waves deal that CU's row groups; small
// problems (fewer groups than one 256-thread block per CU would hold) keep one 256-thread block per 4 groups and the plain walk (*ncu_out = 0)
static inline int balanced_grid(int n_groups, int* ncu_out, int* per_out, int max_per = GEMV_BPC) {
    const int ncu = gemv_cu_count();
    int want = cdiv(n_groups, 4);
    if (want <= ncu) {
        *ncu_out = 0; *per_out = 1;
        return want;
    }
    int per = cdiv(want, ncu); if (per > max_per) per = max_per;
    *ncu_out = ncu; *per_out = per;
    return ncu;
}
int gemv_grid_blocks(int N) {
    int ncu = 0, per = 1;
    return balanced_grid(cdiv(N, 2), &ncu, &per);
}

// The kernel's arguments from GemvArgs: the flat head (per mode, see gemv_kernel), the map planned here once per launch, the tail.
template <int MODE, int U>
static void gemv_launch(int per, int grid, size_t lds, hipStream_t s, const GemvArgs& a, int n_groups, int ncu, int skew) {
    const void* a1 = MODE == 2 ? (const void*)a.part_o : (const void*)a.x;
    const void* a2 = MODE == 2 ? (const void*)a.part_ml : MODE == 1 ? (const void*)a.W2 : (const void*)a.norm_w;
    const void* a3 = MODE == 2 ? (const void*)a.pos_ptr : MODE == 1 ? (const void*)a.norm_w : nullptr;
    GemvPlan pl{0, grid * 4, 0};                                  // small grids: 256-thread blocks walk with stride blocks x 4 waves
    if (ncu > 0) pl = gemv_plan(n_groups, ncu, skew);
    const GemvTail t{a.bias, a.residual, a.y, a.y_f32, a.amax_v, a.amax_i, a.eps, a.split_keys};
#define GEMV_GO(NT)                                                                                                                                  \
    do {                                                                                                                                             \
        if constexpr (gemv_flat_head(MODE, U))                                                                                                       \
            hipLaunchKernelGGL((gemv_kernel<MODE, U, NT>), dim3(grid), dim3(NT), lds, s, a.W, a1, a2, a3, a.K, a.N, a.n_splits, pl.ncu_xr, pl.cf, pl.xq, t); \
        else                                                                                                                                         \
            hipLaunchKernelGGL((gemv_kernel_args<MODE, U, NT>), dim3(grid), dim3(NT), lds, s, a, n_groups, ncu, skew);                               \
    } while (0)
    if constexpr (MODE == 2) {   // 8 waves per CU at most (launch_gemv asks balanced_grid for per <= 2): the wider blocks are not built
        if (per == 1) GEMV_GO(256); else GEMV_GO(512);
    } else switch (per) {
        case 1: GEMV_GO(256); break;
        case 2: GEMV_GO(512); break;
        case 3: GEMV_GO(768); break;
        default: GEMV_GO(1024); break;
    }
#undef GEMV_GO
}

int launch_gemv(const GemvArgs& a, hipStream_t s) {
    VILA_REQUIRE(a.K % 8 == 0 && a.K > 0 && a.N > 0, "gemv: K=%d must be a positive multiple of 8", a.K);
    VILA_REQUIRE((uintptr_t)a.W % 16 == 0, "gemv: weight pointer alignment");
    VILA_REQUIRE(a.amax_v == nullptr || (a.mode == 0 && a.y_f32 != nullptr && a.amax_i != nullptr), "gemv: the fused pick needs mode 0 with fp32 output");
    const int n_groups = cdiv(a.N, 2);
    int ncu = 0, per = 1;
    // mode 2: 8 waves per CU at most (the merge prologue; measured best)
    const int grid = balanced_grid(n_groups, &ncu, &per, a.mode == 2 ? 2 : GEMV_BPC);
    VILA_REQUIRE(ncu <= GEMV_PLAN_MAX_CUS, "gemv: the CU map holds up to %d CUs (got %d)", GEMV_PLAN_MAX_CUS, ncu);
    size_t lds = ((size_t)a.K * 2 + 15) / 16 * 16 + 16;
    const bool short_k = a.K <= 3584;
    if (a.mode == 1) {
        VILA_REQUIRE(a.W2 != nullptr && a.y != nullptr && (uintptr_t)a.x % 16 == 0, "gemv: gate/up mode needs W2, bf16 y, aligned x");
        // skew 1: one gate/up group per CU moves from the odd XCDs to the even ones (profiles/r06_gemv_cu_map_ab.log: 337.8 -> 339.3 tok/s)
        gemv_launch<1, 4>(per, grid, lds, s, a, n_groups, ncu, 1);
    } else if (a.mode == 2) {
        VILA_REQUIRE(a.part_o != nullptr && a.part_ml != nullptr && a.pos_ptr != nullptr && a.K % 128 == 0, "gemv: attention-merge mode needs partials");
        VILA_REQUIRE(a.n_splits >= 1 && a.n_splits <= MERGE_MAXS, "gemv: the merge prologue holds 1..%d slices (got %d)", MERGE_MAXS, a.n_splits);
        VILA_REQUIRE(a.K / 128 <= 256, "gemv: the merge prologue forms one head's weights per thread of its smallest block: up to 256 heads (got %d)", a.K / 128);
        lds += (size_t)a.n_splits * (a.K / 128) * 4;
        if (short_k) gemv_launch<2, 7>(per, grid, lds, s, a, n_groups, ncu, 0);
        else gemv_launch<2, 4>(per, grid, lds, s, a, n_groups, ncu, 0);
    } else {
        VILA_REQUIRE((uintptr_t)a.x % 16 == 0, "gemv: x alignment");
        if (short_k) gemv_launch<0, 7>(per, grid, lds, s, a, n_groups, ncu, 0);
        else gemv_launch<0, 4>(per, grid, lds, s, a, n_groups, ncu, 0);
    }
    VILA_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// fused RMSNorm + QKV projection + bias + RoPE + KV-cache append for one new token.
// Group = 2 rows per wave: q/k heads -> the rotate-half pair {d, d+hd/2} of one head, v heads -> 2 consecutive rows.  cos/sin of the token's position come from the per-token table written by
// decode_prologue_kernel (already rounded to bf16 like HF's cast of cos/sin to the activation dtype).
// ------------------------------------------------------------------------------------------------
// Arguments as in gemv_kernel: the weights, x, the gain, K, the head geometry and the CU map flat in front (14 dwords, preloaded); the rest in
// QkvTail, fetched behind the first weight batch.  A row group splits into (head, pair) by a multiplication (gph_magic: gemv_plan.h udiv_magic).
struct QkvTail {
    const bf16_t* bqkv; bf16_t* q_out; bf16_t* kcache; bf16_t* vcache; const int32_t* pos_ptr; const float* rope_cs;
    float eps; int max_ctx;
};
__device__ __forceinline__ void tail_here(const QkvTail& t) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" :: "s"(t.bqkv), "s"(t.q_out), "s"(t.kcache), "s"(t.vcache), "s"(t.pos_ptr), "s"(t.rope_cs), "s"(t.eps), "s"(t.max_ctx));
    __builtin_amdgcn_sched_barrier(0);
}
template <int U, int NT>
__global__ __launch_bounds__(NT) void qkv_decode_kernel(const bf16_t* Wqkv, const bf16_t* x, const bf16_t* norm_w, int K, int hd, int nq, int nkv,
                                                        unsigned gph_magic, int ncu_xr, int cf, int xq, QkvTail t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* sx = (bf16_t*)smem;
    float* scratch = (float*)(smem + ((K * 2 + 15) & ~15));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = hd >> 1;
    const int gph = half;                                      // groups (row pairs) per head
    const int n_groups = (nq + 2 * nkv) * gph;
    const int nch = K >> 3;
    constexpr int WPB = NT / 64;
    constexpr bool CW = qkv_counted_waits(U), XS = qkv_tail_dpp(U);
    const GemvPlan cm{ncu_xr, cf, xq};
    const int ncu = cm.ncu();
    const int cu = ncu > 0 ? (int)blockIdx.x : 0;
    const int cnt = ncu > 0 ? cm.count(cu) : 0;
    int j = wave;
    const int stride = cf;                                     // small grids: blocks x WPB
    int g = ncu > 0 ? (j < cnt ? cm.gid(cu, j) : n_groups) : blockIdx.x * WPB + wave;
    auto next_group = [&]() { if (ncu > 0) { j += WPB; g = j < cnt ? cm.gid(cu, j) : n_groups; } else g += stride; };

    int rows_i[2];
    const bf16_t* rows[2];
    auto rows_of = [&](int gg) {
        if constexpr (CW) gg = __builtin_amdgcn_readfirstlane(gg);   // as in gemv_body
        const int head = (int)udiv_by_magic((unsigned)gg, gph_magic), gi = gg - head * gph;
        if (head >= nq + nkv) { rows_i[0] = head * hd + gi * 2; rows_i[1] = rows_i[0] + 1; }   // v: two consecutive rows
        else { rows_i[0] = head * hd + gi; rows_i[1] = rows_i[0] + half; }                        // q/k: the rotate-half pair (d, d + hd/2)
        rows[0] = Wqkv + (int64_t)rows_i[0] * K;
        rows[1] = Wqkv + (int64_t)rows_i[1] * K;
    };
    // epilogue operands (position, the pair's biases, its RoPE row) are requested before the dot product, not after the reduction
    int e_pos = 0;
    bf16_t e_b0 = 0, e_b1 = 0;                       // as loaded (bf2f_late)
    float e_c = 1.f, e_s = 0.f;
    auto epi_fetch = [&](int gg) {
        if (lane >= 2) return;
        const int head = (int)udiv_by_magic((unsigned)gg, gph_magic), gi = gg - head * gph;
        e_pos = *t.pos_ptr;
        e_b0 = t.bqkv != nullptr ? t.bqkv[rows_i[0]] : (bf16_t)0;
        e_b1 = t.bqkv != nullptr ? t.bqkv[rows_i[1]] : (bf16_t)0;
        if (head < nq + nkv) { e_c = t.rope_cs[gi]; e_s = t.rope_cs[half + gi]; }
    };
    auto finish = [&](int gg, float (&acc)[2]) {
        if (lane >= 2) return;
        const int head = (int)udiv_by_magic((unsigned)gg, gph_magic);
        const bool is_v = head >= nq + nkv;
        const int pos = e_pos;
        const float lo = bfround(acc[0] + bf2f_late(e_b0));
        const float hi = bfround(acc[1] + bf2f_late(e_b1));
        float out = lane ? hi : lo;
        if (!is_v) {
            const float c = e_c, sn = e_s;
            out = lane ? bfround(bfround(hi * c) + bfround(lo * sn)) : bfround(bfround(lo * c) + bfround(-hi * sn));
        }
        const int row = rows_i[lane];
        if (head < nq) {
            t.q_out[row] = f2bf(out);
        } else if (pos < t.max_ctx) {
            const int kvh = is_v ? head - nq - nkv : head - nq;
            bf16_t* dst = (is_v ? t.vcache : t.kcache) + ((int64_t)kvh * t.max_ctx + pos) * hd;
            dst[row - head * hd] = f2bf(out);
        }
    };

    Batch<2, U> b0;
    const bool has = g < n_groups;
    if (has) { rows_of(g); load_batch<2, U>(rows, 0, lane, nch, b0); }
    tail_here(t);
    if (has) epi_fetch(g);   // weights in front (gemv_kernel: no gain from the inputs first)
    STAGE_X_REGS(NT, st);
    stage_x_issue<NT>(x, norm_w, K, STAGE_X_ARGS(st));
    stage_x_finish<NT, true, XS>(x, norm_w, t.eps, K, sx, scratch, STAGE_X_ARGS(st));   // LDS-only syncs: measured faster here (CHANGELOG)
    if (has) {
        float acc[2] = {0.f, 0.f};
        if constexpr (CW) fma_batch_any<2, U>(b0, sx, 0, lane, nch, acc); else fma_batch<2, U>(b0, sx, 0, lane, nch, acc);
        wave_rows_dot<2, U, CW, XS>(rows, sx, K, lane, acc, 64 * U);
        finish(g, acc);
        next_group();
    }
    for (; g < n_groups; next_group()) {
        rows_of(g);
        epi_fetch(g);
        float acc[2] = {0.f, 0.f};
        wave_rows_dot<2, U, CW, XS>(rows, sx, K, lane, acc, 0);
        finish(g, acc);
    }
}

template <int U>
static void qkv_launch(int per, int grid, size_t lds, hipStream_t s, const QkvDecodeArgs& a, int n_groups, int ncu) {
    GemvPlan pl{0, grid * 4, 0};                                  // small grids: 256-thread blocks walk with stride blocks x 4 waves
    if (ncu > 0) pl = gemv_plan(n_groups, ncu, 0);
    const unsigned magic = udiv_magic((unsigned)(a.hd / 2));
    const QkvTail t{a.bqkv, a.q_out, a.kcache, a.vcache, a.pos_ptr, a.rope_cs, a.eps, a.max_ctx};
#define QKV_GO(NT) hipLaunchKernelGGL((qkv_decode_kernel<U, NT>), dim3(grid), dim3(NT), lds, s, a.Wqkv, a.x, a.norm_w, a.K, a.hd, a.nq, a.nkv, magic, pl.ncu_xr, pl.cf, pl.xq, t)
    switch (per) {
        case 1: QKV_GO(256); break;
        case 2: QKV_GO(512); break;
        case 3: QKV_GO(768); break;
        default: QKV_GO(1024); break;
    }
#undef QKV_GO
}
int launch_qkv_decode(const QkvDecodeArgs& a, hipStream_t s) {
    VILA_REQUIRE(a.K % 8 == 0 && a.hd % 4 == 0 && a.hd > 0 && a.rope_cs != nullptr, "qkv_decode: K=%d hd=%d", a.K, a.hd);
    const int n_groups = (a.nq + 2 * a.nkv) * (a.hd / 2);
    VILA_REQUIRE(n_groups > 0 && (uint64_t)n_groups * (uint64_t)(a.hd / 2) < (1ull << 32), "qkv_decode: %d row groups of %d per head", n_groups, a.hd / 2);
    const size_t lds = ((size_t)a.K * 2 + 15) / 16 * 16 + 16;
    // one rotate-half pair per wave; K <= 3584: the whole row pair (14 x 16 B per lane) is in flight in ONE round trip
    int ncu = 0, per = 1;
    const int grid = balanced_grid(n_groups, &ncu, &per);
    VILA_REQUIRE(ncu <= GEMV_PLAN_MAX_CUS, "qkv_decode: the CU map holds up to %d CUs (got %d)", GEMV_PLAN_MAX_CUS, ncu);
    if (a.K <= 3584) qkv_launch<7>(per, grid, lds, s, a, n_groups, ncu);
    else qkv_launch<4>(per, grid, lds, s, a, n_groups, ncu);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// probe of the two wave reductions (tests/test_gpu_decode_tail.py): one wave per 64 inputs, every lane writes what each butterfly leaves it
__global__ __launch_bounds__(64) void wave_sum_probe_kernel(const float* __restrict__ in, float* __restrict__ out_xor, float* __restrict__ out_shfl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const float v = in[i];
    out_xor[i] = wave_sum_xor(v);
    out_shfl[i] = wave_sum(v);
}
int launch_wave_sum_probe(const float* in, float* out_xor, float* out_shfl, int n_waves, hipStream_t s) {
    VILA_REQUIRE(n_waves > 0 && in != nullptr && out_xor != nullptr && out_shfl != nullptr, "wave_sum_probe: %d waves", n_waves);
    hipLaunchKernelGGL(wave_sum_probe_kernel, dim3(n_waves), dim3(64), 0, s, in, out_xor, out_shfl);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// per-token prologue: x = embed[token]; rope table for the token's position: cs[0:hd/2] = cos, cs[hd/2:hd] = sin,
// both rounded to bf16 (HF casts cos/sin to the activation dtype before use)
__global__ void decode_prologue_kernel(const bf16_t* __restrict__ table, const int64_t* __restrict__ tok, bf16_t* __restrict__ out, int H,
                                       int64_t vocab, const int32_t* __restrict__ pos, float* __restrict__ rope_cs, int hd, float theta) {
    int64_t id = *tok;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < (H >> 3); c += gridDim.x * blockDim.x)
        *(u32x4*)(out + c * 8) = *(const u32x4*)(table + id * H + c * 8);
    if (blockIdx.x == 0 && (int)threadIdx.x < (hd >> 1)) {
        const int d = threadIdx.x;
        const float inv = 1.0f / powf(theta, (float)(2 * d) / (float)hd);
        const float ang = (float)(*pos) * inv;
        rope_cs[d] = bfround(cosf(ang));
        rope_cs[(hd >> 1) + d] = bfround(sinf(ang));
    }
}
int launch_decode_prologue(const bf16_t* table, const int64_t* tok, bf16_t* out, int H, int64_t vocab, const int32_t* pos, float* rope_cs,
                           int hd, float theta, hipStream_t s) {
    VILA_REQUIRE(hd / 2 <= 256, "decode_prologue: head_dim too large");
    hipLaunchKernelGGL(decode_prologue_kernel, dim3(cdiv(H / 8, 256)), dim3(256), 0, s, table, tok, out, H, vocab, pos, rope_cs, hd, theta);
    VILA_LAUNCH_CHECK();
    return 0;
}
__global__ void decode_advance_kernel(int32_t* pos, const int64_t* tok, int64_t* out_ids, int32_t* n_out, int max_out) {
    const int n = *n_out;
    if (n < max_out) out_ids[n] = *tok;
    *n_out = n + 1;
    *pos = *pos + 1;
}
int launch_decode_advance(int32_t* pos, const int64_t* tok, int64_t* out_ids, int32_t* n_out, int max_out, hipStream_t s) {
    hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(1), 0, s, pos, tok, out_ids, n_out, max_out);
    VILA_LAUNCH_CHECK();
    return 0;
}

// Decode attention (q_len = 1, GQA, head_dim 128) of the batch-1 step (api.hip decode_step_impl) and of the batched step (decode_batch.hip):
//   * batch 1, caches up to DEC_SHORT_CTX positions: attn_decode_head, one block of 16 waves per query head; with 256-key slices (the default) its
//     partials are merged in the prologue of the o_proj GEMV (attn_decode.h attn_merge_weights; gemv.hip stage_x_attn, gemv_w4.hip stage_x_attn_w4);
//   * batch 1, longer caches: attn_decode_partial + attn_decode_merge, 64-key split-KV with a merge launch;
//   * the batch: bdec_attn_kernel (one 16-key chunk per wave) up to BDEC_SHORT_CTX positions, bdec_attn_walk_kernel (blocks walk the chunks) beyond,
//     both serving a whole GQA group from one K/V read, and bdec_attn_merge_kernel.
#include "attn_decode.h"
#include "gemv_common.h"
#include "gemv_plan.h"
#include "attn_common.h"

typedef __attribute__((address_space(1))) unsigned long long gu64;
__device__ __forceinline__ unsigned long long pack_f2(float a, float b) {
    return (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32);
}

// ------------------------------------------------------------------------------------------------
// split-KV decode attention (q_len = 1, GQA, hd = 128): grid (n_splits, nkv); a block handles the G = nq/nkv query
// heads of one kv head over a 64-key slice of the cache and writes the un-normalised partial O and (m, l).
// The merge over splits is fused into the o_proj GEMV (gemv_kernel<2>).
//   scores : thread = (key, quarter of d): 32 FMAs per head, 2 cross-lane adds
//   P.V    : thread = (4 keys, 8-wide d chunk): 56 accumulators, reduced over the 16 key groups through LDS
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_decode_partial(AttnDecodeArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sq = (float*)smem;                       // [G][128]  (pre-scaled)
    float* sc = sq + DEC_MAXG * 128;                // [G][64]
    float* red = sc + DEC_MAXG * DEC_KS;            // [16][G][128]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x, kvh = blockIdx.y;
    const int G = p.nq / p.nkv;
    const int nkeys = *p.pos_ptr + 1;
    const int k0 = split * DEC_KS;
    if (k0 >= nkeys) return;
    const int kn = (nkeys - k0) < DEC_KS ? (nkeys - k0) : DEC_KS;
    const bf16_t* kb = p.kcache + ((int64_t)kvh * p.max_ctx + k0) * 128;
    const bf16_t* vb = p.vcache + ((int64_t)kvh * p.max_ctx + k0) * 128;

    const int kq = tid >> 2, qd = tid & 3;          // scores: key, d quarter
    const int vkg = tid >> 4, vch = tid & 15;       // P.V: key group (4 keys), d chunk
    u32x4 kv_[4], vv_[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kv_[j] = (kq < kn) ? *(const u32x4*)(kb + kq * 128 + qd * 32 + j * 8) : (u32x4){0u, 0u, 0u, 0u};
        const int key = vkg * 4 + j;
        vv_[j] = (key < kn) ? *(const u32x4*)(vb + key * 128 + vch * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
    for (int i = tid; i < G * 128; i += 256) sq[i] = bf2f(p.q[kvh * G * 128 + i]) * p.scale;
    __syncthreads();

    for (int g = 0; g < G; ++g) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 q0 = *(const f32x4*)(sq + g * 128 + qd * 32 + j * 8);
            const f32x4 q1 = *(const f32x4*)(sq + g * 128 + qd * 32 + j * 8 + 4);
            a = fmaf(lo_bf(kv_[j][0]), q0[0], a); a = fmaf(hi_bf(kv_[j][0]), q0[1], a);
            a = fmaf(lo_bf(kv_[j][1]), q0[2], a); a = fmaf(hi_bf(kv_[j][1]), q0[3], a);
            a = fmaf(lo_bf(kv_[j][2]), q1[0], a); a = fmaf(hi_bf(kv_[j][2]), q1[1], a);
            a = fmaf(lo_bf(kv_[j][3]), q1[2], a); a = fmaf(hi_bf(kv_[j][3]), q1[3], a);
        }
        a += __shfl_xor(a, 1, 64);
        a += __shfl_xor(a, 2, 64);
        if (qd == 0) sc[g * DEC_KS + kq] = kq < kn ? a : -INFINITY;
    }
    __syncthreads();

    for (int g = wave; g < G; g += 4) {             // softmax statistics: one wave per head, lane = key
        const float s = sc[g * DEC_KS + lane];
        const float m = wave_max(s);
        const float e = __expf(s - m);
        const float l = wave_sum(e);
        sc[g * DEC_KS + lane] = e;
        if (lane == 0) {
            // (m, l) as ONE 8-byte write-through (sc1) store: the combine below reads it with sc1 loads, no fences needed
            gu64* ml = (gu64*)(p.part_ml + ((int64_t)split * p.nq + kvh * G + g) * 2);
            __hip_atomic_store(ml, pack_f2(m, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();

    for (int g = 0; g < G; ++g) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float pr = sc[g * DEC_KS + vkg * 4 + j];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[2 * k] = fmaf(pr, lo_bf(vv_[j][k]), o[2 * k]);
                o[2 * k + 1] = fmaf(pr, hi_bf(vv_[j][k]), o[2 * k + 1]);
            }
        }
        float* r = red + ((vkg * G + g) * 128 + vch * 8);
        *(f32x4*)r = (f32x4){o[0], o[1], o[2], o[3]};
        *(f32x4*)(r + 4) = (f32x4){o[4], o[5], o[6], o[7]};
    }
    __syncthreads();
    // partial O as 8-byte write-through (sc1) stores (guide G16 R1: payload sc1 -> every storing wave drains -> flag)
    for (int i = tid; i < G * 64; i += 256) {
        float o0 = 0.f, o1 = 0.f;
#pragma unroll
        for (int kg = 0; kg < 16; ++kg) { o0 += red[kg * G * 128 + 2 * i]; o1 += red[kg * G * 128 + 2 * i + 1]; }
        gu64* dst = (gu64*)(p.part_o + ((int64_t)split * p.nq + kvh * G) * 128 + 2 * i);
        __hip_atomic_store(dst, pack_f2(o0, o1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// merge of the split partials.  Measured alternatives (profiles/r01 notes in DESIGN.md §4.3): combine by the last-arriving
// block inside the partial kernel (fences: 14.6 us, sc1 stores+loads: 16.3 us) and combine inside the o_proj GEMV prologue
// (18.0 us for o_proj) are all no faster than this separate 7 us launch, so the simplest form is kept.
__global__ __launch_bounds__(128) void attn_decode_merge(AttnDecodeArgs p) {
    const int h = blockIdx.x, d = threadIdx.x;
    const int nkeys = *p.pos_ptr + 1;
    const int ns = (nkeys + DEC_KS - 1) / DEC_KS;
    float M = -INFINITY;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, p.part_ml[((int64_t)s * p.nq + h) * 2]);
    float L = 0.f, o = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float* ml = p.part_ml + ((int64_t)s * p.nq + h) * 2;
        const float w = __expf(ml[0] - M);
        L += w * ml[1];
        o += w * p.part_o[((int64_t)s * p.nq + h) * 128 + d];
    }
    p.o[h * 128 + d] = f2bf(o / L);
}

// ------------------------------------------------------------------------------------------------
// single-launch decode attention for short contexts (cache capacity <= DEC_SHORT_CTX): one block of 16 waves per QUERY head walks the
// whole context (wave w takes 16-key chunks w, w+16, ...), online softmax per wave, cross-wave merge in LDS.  No split-KV
// partials and no merge launch: 2 launches -> 1 per layer (each launch costs ~3-4 us of floor inside the decode graph); the
// price is that the G = 7 query heads of a kv head each read that head's K/V (served by L2 / MALL, 2.5 % of a token's bytes).
//   scores: lane = (key = lane/4, d quarter = lane%4): 32 FMAs + 2 cross-lane adds;  P.V: lane = (4-key subgroup, 8-wide d chunk)
// ------------------------------------------------------------------------------------------------
// SPLIT: grid (nq, ceil(max_ctx / 256)); block (h, s) covers keys [256 s, 256 s + 256) — ONE 16-key chunk per wave, no loop — and writes the
// un-normalised partial (o, m, l) of that slice; the merge over the <= 8 slices happens in the o_proj GEMV's prologue (gemv_kernel<2>).
// Arguments ("the head of a kernel"): what the first requests need — q, the caches, the position, the row strides of the batched
// form, the capacity and the kv head of a query head as a multiplication (kvh_magic: gemv_plan.h udiv_magic of the GQA group, 0 for a group of
// one) — flat in front, 14 dwords that the wave finds in SGPRs at its start (kernarg preload; vila_amd/build.py); the rest in AttnHeadTail,
// fetched behind the first K/V chunk.
struct AttnHeadTail { bf16_t* o; float* part_o; float* part_ml; int64_t o_row_stride; int nq; float scale; };
template <bool SPLIT>
__global__ __launch_bounds__(1024) void attn_decode_head(const bf16_t* q, const bf16_t* kcache, const bf16_t* vcache, const int32_t* pos_ptr,
                                                         int64_t q_row_stride, int64_t slot_stride, int max_ctx, unsigned kvh_magic, AttnHeadTail t) {
    __shared__ float sq[128];
    __shared__ float so[16][128];
    __shared__ float sml[16][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, kvh = kvh_magic ? (int)udiv_by_magic((unsigned)h, kvh_magic) : h;
    const int key_lo = SPLIT ? blockIdx.y * 256 : 0;
    const int row = blockIdx.z;                                  // batched decode: sequence = cache slot (0 for the batch-1 step)
    q += row * q_row_stride; kcache += row * slot_stride; vcache += row * slot_stride;
    const bf16_t* kb = kcache + (int64_t)kvh * max_ctx * 128;
    const bf16_t* vb = vcache + (int64_t)kvh * max_ctx * 128;
    const int kq = lane >> 2, qd = lane & 3;        // scores: key within the chunk, d quarter
    const int sg = lane >> 4, dc = lane & 15;       // P.V: 4-key subgroup, d chunk
    u32x4 kc[4], vc[4], kn_[4], vn_[4];
    // The order of the prologue: q, the position and the wave's first K/V chunk are requested together; none needs another and
    // none is predicated (straight-line code: the wait in front of the LDS write of q is a count that leaves K/V in flight).  The chunk's loads
    // know only the CAPACITY yet: a key at or past max_ctx is clamped to the cache's last row (a cache of 300 positions is never read at row
    // 300).  Once the position is here, the rows at or past nkeys, which may hold anything, are replaced by the zero vectors that a load
    // predicated on nkeys produces.
    int k0 = key_lo + wave * 16;
    const int nkeys_all = pos_ptr[row] + 1;
    const bf16_t qv = q[h * 128 + (tid & 127)];
    __builtin_amdgcn_sched_barrier(0);                           // the small loads stay in front of K/V ...
    {
        const int cap = max_ctx - 1;
        const int key = k0 + kq < cap ? k0 + kq : cap;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kc[j] = *(const u32x4*)(kb + (int64_t)key * 128 + qd * 32 + j * 8);
            const int vk = k0 + sg * 4 + j < cap ? k0 + sg * 4 + j : cap;
            vc[j] = *(const u32x4*)(vb + (int64_t)vk * 128 + dc * 8);
        }
    }
    __builtin_amdgcn_sched_barrier(0);                           // ... and in front of the return below, which waits for the position
    asm volatile("" :: "s"(t.o), "s"(t.part_o), "s"(t.part_ml), "s"(t.o_row_stride), "s"(t.nq), "s"(t.scale));   // the tail's scalar loads: here
    __builtin_amdgcn_sched_barrier(0);
    if (SPLIT && key_lo >= nkeys_all) return;                    // block-uniform: slices beyond the context write nothing (the merge skips them)
    const int nkeys = SPLIT ? (nkeys_all < key_lo + 256 ? nkeys_all : key_lo + 256) : nkeys_all;
    auto load_chunk = [&](int k0, u32x4 (&kk)[4], u32x4 (&vv)[4]) {
        const int key = k0 + kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kk[j] = (key < nkeys) ? *(const u32x4*)(kb + (int64_t)key * 128 + qd * 32 + j * 8) : (u32x4){0u, 0u, 0u, 0u};
            const int vk = k0 + sg * 4 + j;
            vv[j] = (vk < nkeys) ? *(const u32x4*)(vb + (int64_t)vk * 128 + dc * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    if (tid < 128) sq[tid] = bf2f(qv) * t.scale;
    sync_lds();                                                  // LDS only: a __syncthreads() would drain the K/V loads (gemv_common.h)
    float qr[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) qr[i] = sq[qd * 32 + i];
    float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (k0 + kq >= nkeys) kc[j] = (u32x4){0u, 0u, 0u, 0u};
        if (k0 + sg * 4 + j >= nkeys) vc[j] = (u32x4){0u, 0u, 0u, 0u};
        kn_[j] = (u32x4){0u, 0u, 0u, 0u}; vn_[j] = (u32x4){0u, 0u, 0u, 0u};
    }
    for (; k0 < nkeys; k0 += 256) {
        const int kn = k0 + 256;
        // prefetch the wave's next chunk under this chunk's math (a 256-key slice is one chunk per wave: nothing follows)
        if (!SPLIT && kn < nkeys) load_chunk(kn, kn_, vn_);
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a = fmaf(lo_bf(kc[j][e]), qr[j * 8 + 2 * e], a);
                a = fmaf(hi_bf(kc[j][e]), qr[j * 8 + 2 * e + 1], a);
            }
        a += __shfl_xor(a, 1, 64);
        a += __shfl_xor(a, 2, 64);
        const float s = (k0 + kq < nkeys) ? a : -INFINITY;
        float cm = s;
        cm = fmaxf(cm, __shfl_xor(cm, 4, 64)); cm = fmaxf(cm, __shfl_xor(cm, 8, 64));
        cm = fmaxf(cm, __shfl_xor(cm, 16, 64)); cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
        const float m_new = fmaxf(m, cm);
        const float alpha = __expf(m - m_new);
        const float pr = __expf(s - m_new);
        float ps = pr;
        ps += __shfl_xor(ps, 4, 64); ps += __shfl_xor(ps, 8, 64); ps += __shfl_xor(ps, 16, 64); ps += __shfl_xor(ps, 32, 64);
        l = l * alpha + ps;
        m = m_new;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] *= alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float pj = __shfl(pr, (sg * 4 + j) * 4, 64);   // probability of key k0 + sg*4 + j (held by lanes 4*key .. 4*key+3)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[2 * e] = fmaf(pj, lo_bf(vc[j][e]), o[2 * e]);
                o[2 * e + 1] = fmaf(pj, hi_bf(vc[j][e]), o[2 * e + 1]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { kc[j] = kn_[j]; vc[j] = vn_[j]; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { o[e] += __shfl_xor(o[e], 16, 64); o[e] += __shfl_xor(o[e], 32, 64); }
    if (lane < 16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) so[wave][dc * 8 + e] = o[e];
    }
    if (lane == 0) { sml[wave][0] = m; sml[wave][1] = l; }
    __syncthreads();
    if (tid < 128) {
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 16; ++w) M = fmaxf(M, sml[w][0]);
        float L = 0.f, acc = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const float wgt = __expf(sml[w][0] - M);
            L += wgt * sml[w][1];
            acc += wgt * so[w][tid];
        }
        if (SPLIT) {
            const int64_t slot = (int64_t)blockIdx.y * t.nq + h;
            t.part_o[slot * 128 + tid] = acc;
            if (tid == 0) { t.part_ml[slot * 2] = M; t.part_ml[slot * 2 + 1] = L; }
        } else {
            (t.o + row * t.o_row_stride)[h * 128 + tid] = f2bf(acc / L);
        }
    }
}

// the kernel's arguments from AttnDecodeArgs (nq a multiple of nkv: checked by the callers)
template <bool SPLIT>
static void launch_head(const AttnDecodeArgs& a, dim3 grid, hipStream_t s) {
    const int G = a.nq / a.nkv;
    const AttnHeadTail t{a.o, a.part_o, a.part_ml, a.o_row_stride, a.nq, a.scale};
    hipLaunchKernelGGL(attn_decode_head<SPLIT>, grid, dim3(1024), 0, s, a.q, a.kcache, a.vcache, a.pos_ptr, a.q_row_stride, a.slot_stride, a.max_ctx,
                       G > 1 ? udiv_magic((unsigned)G) : 0u, t);
}

// batched decode: one block per (query head, sequence) over the sequence's whole context (caches up to DEC_SHORT_CTX positions)
int launch_attn_decode_rows(const AttnDecodeArgs& a0, int n_rows, int64_t q_row_stride, int64_t o_row_stride, int64_t slot_stride, hipStream_t s) {
    AttnDecodeArgs a = a0;
    VILA_REQUIRE(a.hd == 128 && a.o != nullptr && a.max_ctx <= DEC_SHORT_CTX && n_rows >= 1, "attn_decode_rows: head_dim 128, caches up to 2048 positions");
    VILA_REQUIRE(a.nq % a.nkv == 0, "attn_decode_rows: q heads must be a multiple of kv heads");
    a.q_row_stride = q_row_stride; a.o_row_stride = o_row_stride; a.slot_stride = slot_stride;
    launch_head<false>(a, dim3(a.nq, 1, n_rows), s);
    VILA_LAUNCH_CHECK();
    return 0;
}

int launch_attn_decode(const AttnDecodeArgs& a, hipStream_t s) {
    VILA_REQUIRE(a.hd == 128, "attn_decode: head_dim must be 128 (got %d)", a.hd);
    VILA_REQUIRE(a.nq % a.nkv == 0 && a.nq / a.nkv <= DEC_MAXG, "attn_decode: GQA group %d/%d unsupported (max %d)", a.nq, a.nkv, DEC_MAXG);
    VILA_REQUIRE(a.n_splits * DEC_KS >= a.max_ctx, "attn_decode: n_splits too small for max_ctx");
    if (a.split256) {                                            // partials per 256-key slice; merged by the o_proj GEMV (mode 2, split_keys 256)
        VILA_REQUIRE(a.max_ctx <= DEC_SHORT_CTX && a.n_splits * DEC_KS >= a.max_ctx, "attn_decode: 256-key slices need max_ctx <= 2048");
        launch_head<true>(a, dim3(a.nq, cdiv(a.max_ctx, 256)), s);
        VILA_LAUNCH_CHECK();
        return 0;
    }
    if (a.o != nullptr && a.max_ctx <= DEC_SHORT_CTX) {
        launch_head<false>(a, dim3(a.nq), s);
        VILA_LAUNCH_CHECK();
        return 0;
    }
    const size_t lds = (size_t)(DEC_MAXG * 128 + DEC_MAXG * DEC_KS + 16 * DEC_MAXG * 128) * 4;
    static bool attr_set = false;
    if (!attr_set) {
        VILA_HIP(hipFuncSetAttribute((const void*)attn_decode_partial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = true;
    }
    hipLaunchKernelGGL(attn_decode_partial, dim3(a.n_splits, a.nkv), dim3(256), lds, s, a);
    VILA_LAUNCH_CHECK();
    if (a.o != nullptr) {
        hipLaunchKernelGGL(attn_decode_merge, dim3(a.nq), dim3(128), 0, s, a);
        VILA_LAUNCH_CHECK();
    }
    return 0;
}

// ---- attention of the batch: one block per (kv head, 256-key slice, sequence) -------------------------------------------------------------
// The batch-1 kernel (attn_decode_head above) gives every QUERY head its own block, so the 7 heads of a GQA group each pull the same
// K/V rows through L2, and a row's whole context is one block's serial loop (19.6 us per layer at 8 x ~800 keys).  Here the K/V chunk a
// wave loads (16 keys) serves all G query heads of its kv head (scores on the matrix core: S[16 keys][16 heads] = K . Q^T in 4 MFMAs; P.V on
// the VALU with the probabilities fetched by DPP row broadcasts, reductions by row swaps — the __shfl_xor formulation, 30 ds_bpermute per
// head, took 69 us), a slice is one chunk per wave (no loop), and the slices are merged by a second small launch.  Merging inside the launch
// (last-arriving block, agent-scope release/acquire by one lane) measured the same 16-17 us total and needs counters; with EVERY wave
// fencing it was 59 us (an agent fence is an L2 write-back + invalidate on this multi-XCD part).
// sum over lane l and lane l ^ 16 (resp. l ^ 32) with gfx950's row swaps (see attn_common.h xor16_max): no LDS crossbar, no lgkmcnt
__device__ __forceinline__ float bd_xor16_sum(float x) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float bd_xor32_sum(float x) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
struct BAttnArgs {
    const bf16_t* q; bf16_t* o;                 // [rows][nq*128]
    const bf16_t* kcache; const bf16_t* vcache; // this layer's [slots][nkv][max_ctx][128]
    const int32_t* pos;                         // [rows]: keys 0 .. pos inclusive
    float* part_o; float* part_ml;              // [rows][nkv][NSL][G][128], [rows][nkv][NSL][G][2]
    int nq, nkv, max_ctx, nsl; int64_t row_stride, o_row_stride, slot_stride; float scale;   // row_stride: q rows, o_row_stride: o rows
    // a prefix session (bdec_attn_walk_kernel<G, true>, bdec_attn_prefix_merge_kernel; unread by every other kernel): the shared length, the rows' flags,
    // the prefix phase's partials [rows][nkv][psl][G][128] + [..][2]
    const int32_t* shared_len; const int32_t* uses; const float* pfx_o; const float* pfx_ml; int psl;
};
// the shared length a prefix session's kernels work with: whole chunks inside the slot, whatever the scalar says
__device__ __forceinline__ int bdec_shared_keys(const int32_t* shared_len, int max_ctx) {
    const int S = *shared_len;
    return (S < 0 ? 0 : (S < max_ctx ? S : max_ctx)) & ~255;
}
// the 16 waves' partials (so [16][G][128], sml [16][G][2] in LDS, published by a barrier) -> the slice's partial in the workspace
template <int G>
__device__ __forceinline__ void bdec_slice_partial(const BAttnArgs& p, const float* so, const float* sml, int row, int kvh, int slice, int tid) {
    const int64_t pbase = ((int64_t)(row * p.nkv + kvh) * p.nsl + slice) * G;
    const int g = tid >> 7, d = tid & 127;
    if (g < G) {
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 16; ++w) M = fmaxf(M, sml[(w * G + g) * 2]);
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const float mw = sml[(w * G + g) * 2];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L = fmaf(sml[(w * G + g) * 2 + 1], f, L);
            O = fmaf(so[(w * G + g) * 128 + d], f, O);
        }
        p.part_o[(pbase + g) * 128 + d] = O;
        if (d == 0) { p.part_ml[(pbase + g) * 2] = M; p.part_ml[(pbase + g) * 2 + 1] = L; }
    }
}
template <int G>
__global__ __launch_bounds__(1024) void bdec_attn_kernel(BAttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* so = (float*)smem;                   // [16 waves][G][128]
    float* sml = so + 16 * G * 128;             // [16][G][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kvh = blockIdx.x, slice = blockIdx.y, row = blockIdx.z;
    const int nkeys_all = p.pos[row] + 1;
    const int active = (nkeys_all + 255) >> 8;
    if (slice >= active) return;                                 // block-uniform
    const int key_lo = slice * 256;
    const int nkeys = nkeys_all < key_lo + 256 ? nkeys_all : key_lo + 256;
    const bf16_t* kb = p.kcache + (int64_t)row * p.slot_stride + (int64_t)kvh * p.max_ctx * 128;
    const bf16_t* vb = p.vcache + (int64_t)row * p.slot_stride + (int64_t)kvh * p.max_ctx * 128;
    const bf16_t* qrow = p.q + (int64_t)row * p.row_stride + kvh * G * 128;
    const int l15 = lane & 15, lg = lane >> 4;      // scores: MFMA A rows = keys, B rows = query heads; C: key lg*4 + r, head l15
    const int sg = lane >> 4, dc = lane & 15;       // P.V: 4-key subgroup (= the C layout's row group), d chunk
    // the wave's 16 keys: everything is issued before anything is used
    const int k0 = key_lo + wave * 16;
    u32x4 kc[4], qc[4], vc[4];
    {
        const int key = k0 + l15;
        const bool kok = key < nkeys, qok = l15 < G;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kc[ks] = kok ? *(const u32x4*)(kb + (int64_t)key * 128 + ks * 32 + lg * 8) : (u32x4){0u, 0u, 0u, 0u};
            qc[ks] = qok ? *(const u32x4*)(qrow + l15 * 128 + ks * 32 + lg * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int vk = k0 + sg * 4 + j;
            vc[j] = (vk < nkeys) ? *(const u32x4*)(vb + (int64_t)vk * 128 + dc * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
    }
    // S[key][head] on the matrix core: 4 MFMAs replace G x (64 FMAs + a 4-lane reduction)
    f32x4 sc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kc[ks]), __builtin_bit_cast(bf16x8, qc[ks]), sc, 0, 0, 0);
    float pr[4], m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) { pr[r] = (k0 + lg * 4 + r < nkeys) ? sc[r] * p.scale : -INFINITY; m = fmaxf(m, pr[r]); }
    m = xor32_max(xor16_max(m));                                 // over the 16 keys of the chunk (lanes l15, l15 + 16, + 32, + 48)
    float l = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { pr[r] = (m == -INFINITY) ? 0.f : __expf(pr[r] - m); l += pr[r]; }
    l = bd_xor32_sum(bd_xor16_sum(l));
    if (lg == 0 && l15 < G) { sml[(wave * G + l15) * 2] = m; sml[(wave * G + l15) * 2 + 1] = l; }
    // P.V on the VALU: the probability of (key sg*4 + j, head g) sits in lane 16*sg + g, register j — one DPP row broadcast away
    static_for<0, G>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float pj = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(pr[j]), 0x150 + g, 0xf, 0xf, false));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[2 * e] = fmaf(pj, lo_bf(vc[j][e]), o[2 * e]);
                o[2 * e + 1] = fmaf(pj, hi_bf(vc[j][e]), o[2 * e + 1]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = bd_xor32_sum(bd_xor16_sum(o[e]));
        if (sg == 0) {
            float* dst = so + (wave * G + g) * 128 + dc * 8;
            *(f32x4*)dst = (f32x4){o[0], o[1], o[2], o[3]};
            *(f32x4*)(dst + 4) = (f32x4){o[4], o[5], o[6], o[7]};
        }
    });
    __syncthreads();
    bdec_slice_partial<G>(p, so, sml, row, kvh, slice, tid);
}
// the slices of a (sequence, query head) -> the bf16 attention output; the launch boundary is the publish (no fences)
__global__ __launch_bounds__(128) void bdec_attn_merge_kernel(BAttnArgs p, int G) {
    const int h = blockIdx.x, row = blockIdx.y, d = threadIdx.x;
    const int kvh = h / G, g = h % G;
    const int chunks = (p.pos[row] + 1 + 255) >> 8;
    const int active = chunks < p.nsl ? chunks : p.nsl;         // the walking form: a slice owns chunks s, s + nsl, ...; one without a chunk wrote nothing
    const int64_t b0 = (int64_t)(row * p.nkv + kvh) * p.nsl * G;
    float M = -INFINITY;
    for (int sl = 0; sl < active; ++sl) M = fmaxf(M, p.part_ml[(b0 + sl * G + g) * 2]);
    float L = 0.f, O = 0.f;
    for (int sl = 0; sl < active; ++sl) {
        const float f = __expf(p.part_ml[(b0 + sl * G + g) * 2] - M);
        L = fmaf(p.part_ml[(b0 + sl * G + g) * 2 + 1], f, L);
        O = fmaf(p.part_o[(b0 + sl * G + g) * 128 + d], f, O);
    }
    p.o[(int64_t)row * p.o_row_stride + h * 128 + d] = f2bf(O / L);
}

// ---- the long-context form: blocks WALK ---------------------------------------------------------------------------------------------
// bdec_attn_kernel needs one partial slot per 256-key chunk of the CAPACITY: at 32k positions that is 128 slices per (row, kv head), most of
// them idle for most rows, and a merge over 128 partials.  Here the grid has nsl = min(chunks of the capacity, cap) slices and the block of
// slice s takes chunks s, s + nsl, s + 2 nsl, ... of the row (interleaved: a short row in a long-capacity session still gets one chunk per
// block, a long row spreads evenly).  A wave keeps the chunk's 16 keys, as above, and carries the online softmax across chunks in registers:
// (m, l) of head l15 in every lane, G x 8 fp32 of un-reduced O; a chunk rescales them by exp(m_old - m_new), fetched by the same DPP row
// broadcast as the probabilities.  The cross-lane sums of O and l are linear, so they run once, behind the walk.
// Registers: a 1024-thread block leaves a wave 128.  G x 8 accumulators + Q + K and V of two chunks is 176 at G = 8 (the compiler spilled 156),
// so Q lives in LDS (rows padded for the b128 read), addresses are 32-bit offsets from a uniform base, P.V unpacks one V row at a time, and the
// next chunk's K and V are requested into the registers this chunk's have just left: K behind the 4 score MFMAs, V behind the P.V.  hipcc keeps
// K's request where it is written only while registers allow; at G = 7 / 8 it moves it down to V's (pinning it with a sched_barrier made it spill
// the loaded K, 140 B per lane), and about 10 loop-invariant offsets live in scratch (40 - 56 B per lane; G <= 4: none).  Loads to keys past the
// row's context are redirected to its last key rather than predicated.  The tail is the short form's: 16-wave merge in LDS, partial [rows][nkv][nsl][G][128] + [..][2], merge launch.
// PREFIX (a session with a shared prompt prefix, see bdec_attn_shared_kernel<G, NT, true> below): the private phase.  A row with uses[row] != 0 starts
// behind the shared chunks, c0 = S >> 8, and slice s walks chunks c0 + s, c0 + s + nsl, ... of its own slot; rows 0 .. S - 1 of that slot are never
// read (the redirect of a load past the context goes to the row's LAST key, which is at or behind S).  A row with uses[row] == 0 has c0 = 0 and runs
// the arithmetic of the plain form, operation for operation.
template <int G, bool PREFIX = false>
__global__ __launch_bounds__(1024) void bdec_attn_walk_kernel(BAttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* so = (float*)smem;                   // [16 waves][G][128]
    float* sml = so + 16 * G * 128;             // [16][G][2]
    char* sq = (char*)(sml + 16 * G * 2);       // [16 heads][256 + 16 B], rows >= G zero (the pad of one b128 keeps the fragment read conflict-free)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kvh = blockIdx.x, slice = blockIdx.y, row = blockIdx.z;
    const int pos1 = p.pos[row] + 1;
    const int nkeys = pos1 < p.max_ctx ? pos1 : p.max_ctx;      // never past the slot, whatever the state says
    const int active = (nkeys + 255) >> 8;
    int first = slice;                                           // the slice's first chunk
    if constexpr (PREFIX) first += p.uses[row] != 0 ? bdec_shared_keys(p.shared_len, p.max_ctx) >> 8 : 0;
    if (first >= active) return;                                 // block-uniform: this slice owns no chunk and writes nothing
    const bf16_t* kb = p.kcache + (int64_t)row * p.slot_stride + (int64_t)kvh * p.max_ctx * 128;
    const bf16_t* vb = p.vcache + (int64_t)row * p.slot_stride + (int64_t)kvh * p.max_ctx * 128;
    const bf16_t* qrow = p.q + (int64_t)row * p.row_stride + kvh * G * 128;
    const int l15 = lane & 15, lg = lane >> 4;      // scores: MFMA A rows = keys, B rows = query heads; C: key lg*4 + r, head l15
    const int sg = lane >> 4, dc = lane & 15;       // P.V: 4-key subgroup, d chunk
    const int kw = wave * 16;
    // keys past the row's context (the tail of its last chunk, the chunk requested behind the last one) read the row's LAST key instead: every load
    // is unconditional and finite, the scores of those keys are masked by index, and their probability 0 meets a finite V
    const int last = nkeys - 1;
    // (a uniform base + a 32-bit byte offset per lane: a slot's kv head is at most 32768 x 256 B, and an address costs one register, not two)
    auto load_k = [&](int chunk, u32x4 (&kk)[4]) {
        int key = chunk * 256 + kw + l15;
        key = key < last ? key : last;
        const char* kp = (const char*)kb + (unsigned)(key * 256 + lg * 16);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kk[ks] = *(const u32x4*)(kp + ks * 64);
    };
    auto load_v = [&](int chunk, u32x4 (&vv)[4]) {
        const int v0 = chunk * 256 + kw + sg * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int vk = v0 + j < last ? v0 + j : last;
            vv[j] = *(const u32x4*)((const char*)vb + (unsigned)(vk * 256 + dc * 16));
        }
    };
    u32x4 kc[4], vc[4];
    load_k(first, kc);
    load_v(first, vc);
    if (tid < 256) {
        const int r = tid >> 4, c = tid & 15;
        const u32x4 v = r < G ? *(const u32x4*)(qrow + r * 128 + c * 8) : (u32x4){0u, 0u, 0u, 0u};
        *(u32x4*)(sq + r * 272 + c * 16) = v;
    }
    __syncthreads();
    int qoff = l15 * 272 + lg * 16;
    float m = -INFINITY, l = 0.f, o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
#pragma unroll 1
    for (int chunk = first; chunk < active; chunk += p.nsl) {
        asm volatile("" : "+v"(qoff));                           // keeps the Q fragments in LDS: hoisted out of the loop they cost 16 registers
        f32x4 sc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const u32x4 qc = *(const u32x4*)(sq + qoff + ks * 64);
            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kc[ks]), __builtin_bit_cast(bf16x8, qc), sc, 0, 0, 0);
        }
        load_k(chunk + p.nsl, kc);
        const int k0 = chunk * 256 + kw;
        float pr[4], cm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pr[r] = (k0 + lg * 4 + r < nkeys) ? sc[r] * p.scale : -INFINITY; cm = fmaxf(cm, pr[r]); }
        cm = xor32_max(xor16_max(cm));                           // over the 16 keys of the chunk
        const float m_new = fmaxf(m, cm);
        const bool none = m_new == -INFINITY;                    // no key of this wave yet (only in the row's last chunk)
        const float alpha = none ? 1.f : __expf(m - m_new);      // m = -inf: 0, and there is nothing to rescale
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pr[r] = none ? 0.f : __expf(pr[r] - m_new); ls += pr[r]; }
        l = fmaf(l, alpha, ls);                                  // this lane's 4 keys; the other 12 are added behind the walk
        m = m_new;
        static_for<0, G>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            const float ag = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(alpha), 0x150 + g, 0xf, 0xf, false));
#pragma unroll
            for (int e = 0; e < 8; ++e) o[g][e] *= ag;
        });
        // key-outer, head-inner: one V row is unpacked to 8 floats at a time (head-outer lets the compiler keep all 4 rows unpacked: 32 registers)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float vf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { vf[2 * e] = lo_bf(vc[j][e]); vf[2 * e + 1] = hi_bf(vc[j][e]); }
            static_for<0, G>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                const float pj = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(pr[j]), 0x150 + g, 0xf, 0xf, false));
#pragma unroll
                for (int e = 0; e < 8; ++e) o[g][e] = fmaf(pj, vf[e], o[g][e]);
            });
        }
        load_v(chunk + p.nsl, vc);
    }
    l = bd_xor32_sum(bd_xor16_sum(l));
    if (lg == 0 && l15 < G) { sml[(wave * G + l15) * 2] = m; sml[(wave * G + l15) * 2 + 1] = l; }
    static_for<0, G>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = bd_xor32_sum(bd_xor16_sum(o[g][e]));
        if (sg == 0) {
            float* dst = so + (wave * G + g) * 128 + dc * 8;
            *(f32x4*)dst = (f32x4){o[g][0], o[g][1], o[g][2], o[g][3]};
            *(f32x4*)(dst + 4) = (f32x4){o[g][4], o[g][5], o[g][6], o[g][7]};
        }
    });
    __syncthreads();
    bdec_slice_partial<G>(p, so, sml, row, kvh, slice, tid);
}
// one slice launch (WALK: the long-context form, whose Q rows sit in LDS behind the partials) and the merge launch
template <int G, bool WALK>
static int launch_bdec_attn_t(const BAttnArgs& a, int rows, hipStream_t s) {
    const size_t lds = (size_t)(16 * G * 128 + 16 * G * 2) * 4 + (WALK ? 16 * 272 : 0);
    const auto kernel = WALK ? bdec_attn_walk_kernel<G> : bdec_attn_kernel<G>;
    static bool attr = false;
    if (!attr) {
        VILA_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    hipLaunchKernelGGL(kernel, dim3(a.nkv, a.nsl, rows), dim3(1024), lds, s, a);
    VILA_LAUNCH_CHECK();
    hipLaunchKernelGGL(bdec_attn_merge_kernel, dim3(a.nq, rows), dim3(128), 0, s, a, G);
    VILA_LAUNCH_CHECK();
    return 0;
}
template <int G>
static int launch_bdec_attn_g(const BAttnArgs& a, bool walk, int rows, hipStream_t s) {
    return walk ? launch_bdec_attn_t<G, true>(a, rows, s) : launch_bdec_attn_t<G, false>(a, rows, s);
}
bool bdec_group_ok(int G) { return G == 1 || G == 2 || G == 4 || G == 7 || G == 8; }
// the short form returns 1 when the GQA group size has no instantiation (the caller falls back to the per-head kernel); the walking form refuses
static int launch_bdec_attn(const BAttnArgs& a, bool walk, int rows, hipStream_t s) {
    switch (a.nq / a.nkv) {
        case 1: return launch_bdec_attn_g<1>(a, walk, rows, s);
        case 2: return launch_bdec_attn_g<2>(a, walk, rows, s);
        case 4: return launch_bdec_attn_g<4>(a, walk, rows, s);
        case 7: return launch_bdec_attn_g<7>(a, walk, rows, s);
        case 8: return launch_bdec_attn_g<8>(a, walk, rows, s);
        default: break;
    }
    VILA_REQUIRE(!walk, "batched decode attention: the walking form serves GQA groups of 1, 2, 4, 7 or 8 query heads (got %d)", a.nq / a.nkv);
    return 1;
}

// ---- which form, how many slices ----------------------------------------------------------------------------------------------------
// Up to 2048 positions: the short form, one slice per 256-key chunk of the capacity (<= 8), exactly as before the walking form existed.
// Beyond: the walking form with min(chunks of the capacity, BDEC_SLICE_CAP) slices.  vila_decode_batch_force_slices (tests, the slice-cap
// measurement) asks for the walking form with a given slice count at any capacity.
static int g_bdec_force_slices = 0;
void bdecode_force_slices(int nsl) { g_bdec_force_slices = nsl < 0 ? 0 : nsl; }
BAttnForm bdec_attn_form(int max_ctx) {
    const int chunks = cdiv(max_ctx, 256);
    if (g_bdec_force_slices > 0) {
        const int f = g_bdec_force_slices < BDEC_MAX_SLICES ? g_bdec_force_slices : BDEC_MAX_SLICES;
        return BAttnForm{true, f < chunks ? f : chunks};
    }
    if (max_ctx <= BDEC_SHORT_CTX) return BAttnForm{false, chunks};
    return BAttnForm{true, chunks < BDEC_SLICE_CAP ? chunks : BDEC_SLICE_CAP};
}
// partial slots the workspace holds per (row, query head): 8 up to 2048 positions (the formula the short form always had), else one per
// chunk of the capacity up to the most a session may ever launch
int bdec_ws_slices(int max_ctx) {
    const int chunks = cdiv(max_ctx, 256);
    return max_ctx <= BDEC_SHORT_CTX ? 8 : (chunks < BDEC_MAX_SLICES ? chunks : BDEC_MAX_SLICES);
}
int bdecode_attn_slices(int max_ctx) { const BAttnForm f = bdec_attn_form(max_ctx); return f.walk ? f.nsl : 0; }
size_t bdecode_attn_workspace_bytes(int rows, int nq, int max_ctx) {
    const size_t sl = (size_t)bdec_ws_slices(max_ctx);
    return align_up((size_t)rows * nq * sl * 128 * 4, 256) + align_up((size_t)rows * nq * sl * 2 * 4, 256);
}
// the launches alone, on partials the caller has laid out for f.nsl slices; 1 = the short form has no instantiation for this GQA group, nothing launched
int bdecode_attn_launch(const BAttnForm& f, const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, const int32_t* pos,
                        bf16_t* o, int64_t ldo, int rows, int nq, int nkv, int max_ctx, float scale, float* part_o, float* part_ml, hipStream_t s) {
    if (!f.walk && nq % nkv != 0) return 1;
    BAttnArgs a{};
    a.q = q; a.o = o; a.kcache = kcache; a.vcache = vcache; a.pos = pos; a.part_o = part_o; a.part_ml = part_ml;
    a.nq = nq; a.nkv = nkv; a.max_ctx = max_ctx; a.nsl = f.nsl; a.row_stride = ldq; a.o_row_stride = ldo; a.slot_stride = slot_stride; a.scale = scale;
    return launch_bdec_attn(a, f.walk, rows, s);
}
int bdecode_attn(const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, const int32_t* pos, bf16_t* o, int64_t ldo,
                 int rows, int nq, int nkv, int max_ctx, float scale, void* workspace, size_t workspace_bytes, hipStream_t s) {
    VILA_REQUIRE(q && kcache && vcache && pos && o && workspace, "attn_decode_batch: NULL argument");
    VILA_REQUIRE(rows >= 1 && nkv >= 1 && nq % nkv == 0 && bdec_group_ok(nq / nkv),
                 "attn_decode_batch: rows >= 1 and a GQA group of 1, 2, 4, 7 or 8 query heads per kv head (got %d rows, %d / %d heads)", rows, nq, nkv);
    VILA_REQUIRE(max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX, "attn_decode_batch: caches of 1..%d positions (got %d)", BDEC_MAX_CTX, max_ctx);
    VILA_REQUIRE(ldq % 8 == 0 && ldq >= (int64_t)nq * 128 && ldo >= (int64_t)nq * 128 && (uintptr_t)q % 16 == 0 && (uintptr_t)kcache % 16 == 0 &&
                 (uintptr_t)vcache % 16 == 0 && slot_stride % 8 == 0 && slot_stride >= (int64_t)nkv * max_ctx * 128,
                 "attn_decode_batch: head_dim 128 rows, 16-byte aligned, slots of [kv_heads][max_ctx][128]");
    VILA_REQUIRE(workspace_bytes >= bdecode_attn_workspace_bytes(rows, nq, max_ctx), "attn_decode_batch: workspace too small");
    const BAttnForm f = bdec_attn_form(max_ctx);
    float* part_ml = (float*)((char*)workspace + align_up((size_t)rows * nq * f.nsl * 128 * 4, 256));
    return bdecode_attn_launch(f, q, ldq, kcache, vcache, slot_stride, pos, o, ldo, rows, nq, nkv, max_ctx, scale, (float*)workspace, part_ml, s);
}

// ---- the verify step's form: n rows of ONE sequence share the K/V read -----------------------------------------------------------------
// A speculative step (decode_batch.hip bverify_step) runs n consecutive positions of one sequence in one cache slot: row i holds position pos + i and
// sees keys 0 .. pos + i.  Through the kernels above (slot_stride 0) every row would pull the same K/V through its own blocks.  Here the columns of
// the score tile are (row, head) pairs, col = row * G + head, ceil(n G / 16) tiles of 16, and the 16 keys a wave loads serve all of them:
//   * scores  S[key][col] = K . Q^T, v_mfma_f32_16x16x32_bf16 as above, 4 per column tile; each column masks by its own limit min(pos + row, max_ctx - 1);
//   * P.V on the matrix core.  The VALU form above keeps 8 fp32 of O per head and lane; with up to 128 columns that is 1024 registers.  The C
//     layout of the score tile (lane = column, registers = the lane group's 4 keys) IS the B operand of v_mfma_f32_16x16x16_bf16 (k = 4 keys per
//     lane group), and the V rows a lane loads for the VALU form (4 keys x 8 consecutive d) hold, element e of the 4 keys, its A operand for
//     the 16 outputs d = 8 l15 + e: O^T[d][col] += V^T[d][key] . P^T[key][col], 8 MFMAs per column tile, no cross-lane movement, no LDS, and the
//     accumulator's column is the lane's own softmax column (the rescale is lane-local).  P is rounded to bf16 and l sums the rounded values, so a
//     column's output stays a convex combination of V rows: |o - exact| <= 2^-9 max|V| before the bf16 store;
//   * a block = 8 waves on one (kv head, slice, group of up to 4 column tiles): 128 accumulator registers per lane of the 256 a wave of a
//     512-thread block may hold.  Steps of more than 64 columns (n G > 64) run two blocks per (kv head, slice), so their K/V is read twice, the
//     second time from L2, where the per-row kernels read it n times;
//   * one form, the walking one: slice s takes the 256-key chunks s, s + nsl, ...; wave w the 16-key pieces w and w + 8 of a chunk; online softmax
//     per wave across everything it walks, the waves meet in LDS a column tile at a time, partials [row][nkv][nsl][G][128] + [..][2] as above.
// Invariance: what a column computes depends on its position and head alone.  Every MFMA output element is a sum over k of its own A row and B
// column; the chunks, pieces and slices are fixed by the capacity; a piece past the column's limit (walked for a later row's sake) is exp(-inf) = 0
// times finite V added to O, alpha = 1; a slice past it is skipped by the merge as above.  So the row's place in the step, the number of rows and
// the tile group it lands in change no bit of its output, which is what makes greedy speculation lossless.
typedef __attribute__((ext_vector_type(4))) short bf16x4s;
#define BSH_MAX_TILES 4                  // column tiles (of 16) per block
struct BSharedArgs {
    const bf16_t* q; bf16_t* o;                 // [n][ldq], [n][ldo]
    const bf16_t* kslot; const bf16_t* vslot;   // one layer's slot [nkv][max_ctx][128]
    const int32_t* pos;                         // device scalar: tokens in the cache = position of row 0 (PREFIX: the shared length S)
    float* part_o; float* part_ml;              // [n][nkv][nsl][G][128], [n][nkv][nsl][G][2]
    int n, nq, nkv, max_ctx, nsl; int64_t ldq, ldo; float scale;
};
// PREFIX: the prefix phase of a session whose rows share a prompt prefix (bdecode_prefix_attn below).  The n rows are rows of DIFFERENT sequences; the slot
// is the session's prefix slot, and every column's limit is S - 1: uniform, whole chunks only (S is read on the device and rounded down to a multiple
// of 256 inside the slot; S = 0: every block returns).  Nothing else changes, so the invariance above holds with "position" read as S.
template <int G, int NT, bool PREFIX = false>
__global__ __launch_bounds__(512) void bdec_attn_shared_kernel(BSharedArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* so = (float*)smem;                   // [8 waves][16 cols][128]
    float* sml = so + 8 * 16 * 128;             // [8][16][2]
    char* sq = (char*)(sml + 8 * 16 * 2);       // [NT * 16 cols][256 + 16 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kvh = blockIdx.x, slice = blockIdx.y, col0 = blockIdx.z * (NT * 16);
    const int ncols = p.n * G;
    const int pos0 = PREFIX ? bdec_shared_keys(p.pos, p.max_ctx) - 1 : *p.pos;
    const int hi = PREFIX ? pos0 : (pos0 + p.n - 1 < p.max_ctx - 1 ? pos0 + p.n - 1 : p.max_ctx - 1);      // the last key any row of the step sees
    const int active = (hi >> 8) + 1;
    if (slice >= active || hi < 0) return;                      // block-uniform: this slice owns no chunk and writes nothing
    const bf16_t* kb = p.kslot + (int64_t)kvh * p.max_ctx * 128;
    const bf16_t* vb = p.vslot + (int64_t)kvh * p.max_ctx * 128;
    const int l15 = lane & 15, lg = lane >> 4;
    auto load_k = [&](int k0, u32x4 (&kk)[4]) {                  // scores: A row = key l15, k = 32 ks + 8 lg ..
        int key = k0 + l15;
        key = key < hi ? key : hi;
        const char* kp = (const char*)kb + (unsigned)(key * 256 + lg * 16);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kk[ks] = *(const u32x4*)(kp + ks * 64);
    };
    auto load_v = [&](int k0, u32x4 (&vv)[4]) {                  // P.V: keys 4 lg + j, d = 8 l15 ..
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int vk = k0 + lg * 4 + j < hi ? k0 + lg * 4 + j : hi;
            vv[j] = *(const u32x4*)((const char*)vb + (unsigned)(vk * 256 + l15 * 16));
        }
    };
    // step t of the wave: chunk slice + (t >> 1) nsl, piece wave + 8 (t & 1)
    const int nsteps = 2 * ((active - slice + p.nsl - 1) / p.nsl);
    auto key0 = [&](int t) { return (slice + (t >> 1) * p.nsl) * 256 + (wave + 8 * (t & 1)) * 16; };
    u32x4 kc[4], vc[4];
    load_k(key0(0), kc);
    load_v(key0(0), vc);
    for (int i = tid; i < NT * 16 * 16; i += 512) {              // Q of the block's columns; columns past the step are zero
        const int c = i >> 4, ch = i & 15, col = col0 + c;
        const int row = col / G, g = col - row * G;
        const u32x4 v = col < ncols ? *(const u32x4*)(p.q + (int64_t)row * p.ldq + (kvh * G + g) * 128 + ch * 8) : (u32x4){0u, 0u, 0u, 0u};
        *(u32x4*)(sq + c * 272 + ch * 16) = v;
    }
    __syncthreads();
    int lim[NT];                                                 // the last key the lane's column of tile t sees; -1: no such column
    float m[NT], l[NT];
    f32x4 acc[NT][8];                                            // O^T: [e][r] = O[col t*16 + l15][d = 8 (4 lg + r) + e]
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = col0 + t * 16 + l15, row = col / G;
        lim[t] = col < ncols ? (PREFIX ? hi : (pos0 + row < p.max_ctx - 1 ? pos0 + row : p.max_ctx - 1)) : -1;
        m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t][e] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int qoff = l15 * 272 + lg * 16;
#pragma unroll 1
    for (int st = 0; st < nsteps; ++st) {
        asm volatile("" : "+v"(qoff));                           // keeps the Q fragments in LDS
        const int k0 = key0(st);
        f32x4 sc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const u32x4 qc = *(const u32x4*)(sq + t * 16 * 272 + qoff + ks * 64);
                sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kc[ks]), __builtin_bit_cast(bf16x8, qc), sc[t], 0, 0, 0);
            }
        }
        load_k(key0(st + 1), kc);                                // (past the last step: the clamp makes it a re-read of key `hi`)
        // V^T fragments: element e of the lane's 4 keys
        bf16x4s va[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = e >> 1;
            unsigned lo, hh;
            if (e & 1) { lo = (vc[0][d] >> 16) | (vc[1][d] & 0xffff0000u); hh = (vc[2][d] >> 16) | (vc[3][d] & 0xffff0000u); }
            else { lo = (vc[0][d] & 0xffffu) | (vc[1][d] << 16); hh = (vc[2][d] & 0xffffu) | (vc[3][d] << 16); }
            va[e] = __builtin_bit_cast(bf16x4s, (unsigned long long)lo | ((unsigned long long)hh << 32));
        }
        load_v(key0(st + 1), vc);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float pr[4], cm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr[r] = (k0 + lg * 4 + r <= lim[t]) ? sc[t][r] * p.scale : -INFINITY; cm = fmaxf(cm, pr[r]); }
            cm = xor32_max(xor16_max(cm));                       // over the 16 keys of the piece
            const float m_new = fmaxf(m[t], cm);
            const bool none = m_new == -INFINITY;                // the column has seen no key of this wave yet
            const float alpha = none ? 1.f : __expf(m[t] - m_new);
            float ls = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr[r] = none ? 0.f : bfround(__expf(pr[r] - m_new)); ls += pr[r]; }
            l[t] = fmaf(l[t], alpha, ls);                        // this lane group's 4 keys; the other 12 are added behind the walk
            m[t] = m_new;
            const unsigned p01 = (__float_as_uint(pr[0]) >> 16) | (__float_as_uint(pr[1]) & 0xffff0000u);
            const unsigned p23 = (__float_as_uint(pr[2]) >> 16) | (__float_as_uint(pr[3]) & 0xffff0000u);
            const bf16x4s pb = __builtin_bit_cast(bf16x4s, (unsigned long long)p01 | ((unsigned long long)p23 << 32));
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[t][e] *= alpha;
                acc[t][e] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(va[e], pb, acc[t][e], 0, 0, 0);
            }
        }
    }
    // the 8 waves meet in LDS, one column tile at a time; thread = (column, 4 d)
    const int mc = tid >> 5, md = (tid & 31) * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float lt = bd_xor32_sum(bd_xor16_sum(l[t]));
        if (lg == 0) { sml[(wave * 16 + l15) * 2] = m[t]; sml[(wave * 16 + l15) * 2 + 1] = lt; }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* dst = so + (wave * 16 + l15) * 128 + (lg * 4 + r) * 8;
            *(f32x4*)dst = (f32x4){acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]};
            *(f32x4*)(dst + 4) = (f32x4){acc[t][4][r], acc[t][5][r], acc[t][6][r], acc[t][7][r]};
        }
        __syncthreads();
        const int col = col0 + t * 16 + mc;
        if (col < ncols) {
            const int row = col / G, g = col - row * G;
            float M = -INFINITY;
#pragma unroll
            for (int w = 0; w < 8; ++w) M = fmaxf(M, sml[(w * 16 + mc) * 2]);
            float L = 0.f;
            f32x4 O = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const float mw = sml[(w * 16 + mc) * 2];
                const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
                L = fmaf(sml[(w * 16 + mc) * 2 + 1], f, L);
                const f32x4 ow = *(const f32x4*)(so + (w * 16 + mc) * 128 + md);
                O[0] = fmaf(ow[0], f, O[0]); O[1] = fmaf(ow[1], f, O[1]); O[2] = fmaf(ow[2], f, O[2]); O[3] = fmaf(ow[3], f, O[3]);
            }
            const int64_t pb = ((int64_t)(row * p.nkv + kvh) * p.nsl + slice) * G + g;
            *(f32x4*)(p.part_o + pb * 128 + md) = O;
            if (md == 0) { p.part_ml[pb * 2] = M; p.part_ml[pb * 2 + 1] = L; }
        }
        __syncthreads();
    }
}
// the slices of a (row, query head) -> the bf16 attention output: bdec_attn_merge_kernel with the row's limit taken from the scalar position
__global__ __launch_bounds__(128) void bdec_attn_shared_merge_kernel(BSharedArgs p, int G) {
    const int h = blockIdx.x, row = blockIdx.y, d = threadIdx.x;
    const int kvh = h / G, g = h % G;
    const int ps = *p.pos + row, last = ps < p.max_ctx - 1 ? ps : p.max_ctx - 1;
    if (last < 0) return;
    const int chunks = (last >> 8) + 1;
    const int active = chunks < p.nsl ? chunks : p.nsl;
    const int64_t b0 = (int64_t)(row * p.nkv + kvh) * p.nsl * G;
    float M = -INFINITY;
    for (int sl = 0; sl < active; ++sl) M = fmaxf(M, p.part_ml[(b0 + sl * G + g) * 2]);
    float L = 0.f, O = 0.f;
    for (int sl = 0; sl < active; ++sl) {
        const float f = __expf(p.part_ml[(b0 + sl * G + g) * 2] - M);
        L = fmaf(p.part_ml[(b0 + sl * G + g) * 2 + 1], f, L);
        O = fmaf(p.part_o[(b0 + sl * G + g) * 128 + d], f, O);
    }
    p.o[(int64_t)row * p.ldo + h * 128 + d] = f2bf(O / L);
}
// (PREFIX: the slice launch alone; the prefix session's merge runs behind its private phase)
template <int G, int NT, bool PREFIX>
static int launch_bdec_shared_t(const BSharedArgs& a, int groups, hipStream_t s) {
    const size_t lds = (size_t)(8 * 16 * 128 + 8 * 16 * 2) * 4 + (size_t)NT * 16 * 272;
    static bool attr = false;
    if (!attr) {
        VILA_HIP(hipFuncSetAttribute((const void*)bdec_attn_shared_kernel<G, NT, PREFIX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    hipLaunchKernelGGL((bdec_attn_shared_kernel<G, NT, PREFIX>), dim3(a.nkv, a.nsl, groups), dim3(512), lds, s, a);
    VILA_LAUNCH_CHECK();
    if (PREFIX) return 0;
    hipLaunchKernelGGL(bdec_attn_shared_merge_kernel, dim3(a.nq, a.n), dim3(128), 0, s, a, G);
    VILA_LAUNCH_CHECK();
    return 0;
}
// tiles = ceil(n G / 16) <= 8: up to 4 in one block, more in two blocks of ceil(tiles / 2)
template <int G, bool PREFIX = false>
static int launch_bdec_shared_g(const BSharedArgs& a, hipStream_t s) {
    const int tiles = cdiv(a.n * G, 16), groups = tiles > BSH_MAX_TILES ? 2 : 1, nt = cdiv(tiles, groups);
    switch (nt) {
        case 1: return launch_bdec_shared_t<G, 1, PREFIX>(a, groups, s);
        case 2: return launch_bdec_shared_t<G, 2, PREFIX>(a, groups, s);
        case 3: return launch_bdec_shared_t<G, 3, PREFIX>(a, groups, s);
        default: return launch_bdec_shared_t<G, 4, PREFIX>(a, groups, s);
    }
}
// slices of the verify form at a capacity: the walking form's cap, or what vila_decode_batch_force_slices asks for
int bverify_attn_slices(int max_ctx) {
    const int chunks = cdiv(max_ctx, 256);
    if (g_bdec_force_slices > 0) {
        const int f = g_bdec_force_slices < BDEC_MAX_SLICES ? g_bdec_force_slices : BDEC_MAX_SLICES;
        return f < chunks ? f : chunks;
    }
    return chunks < BDEC_SLICE_CAP ? chunks : BDEC_SLICE_CAP;
}
static int bverify_ws_slices(int max_ctx) { const int chunks = cdiv(max_ctx, 256); return chunks < BDEC_MAX_SLICES ? chunks : BDEC_MAX_SLICES; }
size_t bverify_attn_workspace_bytes(int n, int nq, int max_ctx) {
    const size_t sl = (size_t)bverify_ws_slices(max_ctx);
    return align_up((size_t)n * nq * sl * 128 * 4, 256) + align_up((size_t)n * nq * sl * 2 * 4, 256);
}
int bverify_attn_launch(const bf16_t* q, int64_t ldq, const bf16_t* kslot, const bf16_t* vslot, const int32_t* pos, bf16_t* o, int64_t ldo, int n, int nq,
                        int nkv, int max_ctx, float scale, float* part_o, float* part_ml, hipStream_t s) {
    BSharedArgs a{};
    a.q = q; a.o = o; a.kslot = kslot; a.vslot = vslot; a.pos = pos; a.part_o = part_o; a.part_ml = part_ml;
    a.n = n; a.nq = nq; a.nkv = nkv; a.max_ctx = max_ctx; a.nsl = bverify_attn_slices(max_ctx); a.ldq = ldq; a.ldo = ldo; a.scale = scale;
    switch (nq / nkv) {
        case 1: return launch_bdec_shared_g<1>(a, s);
        case 2: return launch_bdec_shared_g<2>(a, s);
        case 4: return launch_bdec_shared_g<4>(a, s);
        case 7: return launch_bdec_shared_g<7>(a, s);
        case 8: return launch_bdec_shared_g<8>(a, s);
        default: break;
    }
    VILA_REQUIRE(false, "attn_decode_verify: GQA groups of 1, 2, 4, 7 or 8 query heads per kv head (got %d)", nq / nkv);
    return -1;
}
int bverify_attn(const bf16_t* q, int64_t ldq, const bf16_t* kslot, const bf16_t* vslot, const int32_t* pos, bf16_t* o, int64_t ldo, int n, int nq, int nkv,
                 int max_ctx, float scale, void* workspace, size_t workspace_bytes, hipStream_t s) {
    VILA_REQUIRE(q && kslot && vslot && pos && o && workspace, "attn_decode_verify: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 16 && nkv >= 1 && nq % nkv == 0 && bdec_group_ok(nq / nkv),
                 "attn_decode_verify: 1..16 rows and a GQA group of 1, 2, 4, 7 or 8 query heads per kv head (got %d rows, %d / %d heads)", n, nq, nkv);
    VILA_REQUIRE(max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX, "attn_decode_verify: caches of 1..%d positions (got %d)", BDEC_MAX_CTX, max_ctx);
    VILA_REQUIRE(ldq % 8 == 0 && ldq >= (int64_t)nq * 128 && ldo >= (int64_t)nq * 128 && (uintptr_t)q % 16 == 0 && (uintptr_t)kslot % 16 == 0 &&
                 (uintptr_t)vslot % 16 == 0, "attn_decode_verify: head_dim 128 rows, 16-byte aligned, a slot of [kv_heads][max_ctx][128]");
    VILA_REQUIRE(workspace_bytes >= bverify_attn_workspace_bytes(n, nq, max_ctx), "attn_decode_verify: workspace too small");
    const size_t nsl = (size_t)bverify_attn_slices(max_ctx);
    float* part_ml = (float*)((char*)workspace + align_up((size_t)n * nq * nsl * 128 * 4, 256));
    return bverify_attn_launch(q, ldq, kslot, vslot, pos, o, ldo, n, nq, nkv, max_ctx, scale, (float*)workspace, part_ml, s);
}

// ---- a session whose rows share a prompt prefix: one K/V read of the prefix for all rows --------------------------------------------------------
// The session's cache has one slot more than it has rows, the PREFIX SLOT, whose keys 0 .. S - 1 (S a multiple of 256, a device scalar) are the
// common start of every row with uses[row] != 0.  Such a row attends keys 0 .. S - 1 of the prefix slot and keys S .. pos[row] of its own slot
// (pos[row] >= S is the host's duty); positions stay absolute.  A row with uses[row] == 0 is an ordinary row: keys 0 .. pos[row] of its own slot.
// Three launches:
//   prefix   bdec_attn_shared_kernel<G, NT, true>: columns (row, head) of ALL n rows against the prefix slot, every limit S - 1; partials
//            [n][nkv][psl][G][128] + [..][2], psl = bverify_attn_slices(capacity).  Slices at or past S >> 8 return; S = 0: all of them.  The columns of
//            ordinary rows are computed and never read.
//   private  bdec_attn_walk_kernel<G, true>: row i from chunk c0 = uses[i] ? S >> 8 : 0; partials [n][nkv][nsl][G][128] + [..][2], nsl =
//            bdec_attn_form(capacity).nsl.  Always the walking form (the force hook shows it valid at every capacity).
//   merge    bdec_attn_prefix_merge_kernel: for a sharing row the min(S >> 8, psl) prefix slices, then the min(chunks - c0, nsl) private slices that own
//            a chunk; for an ordinary row the private slices alone.  It reads exactly the partials the two launches above wrote.
// Invariances:
//   (a) a sharing row's output bits do not depend on n, on its row index or on the other rows' flags and positions.  Prefix phase: the shared form's
//       argument — a column's bits depend on its limit (S - 1 for all) and its head, not on the tile group or the column count.  Private phase: a block
//       serves one (row, kv head, slice) and reads that row's q, flag, position and slot alone.  psl and nsl are fixed by the capacity (and the force
//       hook), and the merge walks a row's own partials in a fixed order.
//   (b) an ordinary row gives the bits of vila_attn_decode_batch_bf16 in walking form at the same slice count: c0 = 0 makes the private phase that
//       kernel's arithmetic, and with no prefix slice the merge below is bdec_attn_merge_kernel's loop, operation for operation.
__global__ __launch_bounds__(128) void bdec_attn_prefix_merge_kernel(BAttnArgs p, int G) {
    const int h = blockIdx.x, row = blockIdx.y, d = threadIdx.x;
    const int kvh = h / G, g = h % G;
    const int pos1 = p.pos[row] + 1;
    const int nkeys = pos1 < p.max_ctx ? pos1 : p.max_ctx;
    const int c0 = p.uses[row] != 0 ? bdec_shared_keys(p.shared_len, p.max_ctx) >> 8 : 0;
    const int pact = c0 < p.psl ? c0 : p.psl;                     // prefix slices that own a chunk (none for an ordinary row)
    const int own = ((nkeys + 255) >> 8) - c0;
    const int active = own < p.nsl ? (own < 0 ? 0 : own) : p.nsl; // private slices that own a chunk
    const int64_t a0 = (int64_t)(row * p.nkv + kvh) * p.psl * G;
    const int64_t b0 = (int64_t)(row * p.nkv + kvh) * p.nsl * G;
    float M = -INFINITY;
    for (int sl = 0; sl < pact; ++sl) M = fmaxf(M, p.pfx_ml[(a0 + sl * G + g) * 2]);
    for (int sl = 0; sl < active; ++sl) M = fmaxf(M, p.part_ml[(b0 + sl * G + g) * 2]);
    float L = 0.f, O = 0.f;
    for (int sl = 0; sl < pact; ++sl) {
        const float f = __expf(p.pfx_ml[(a0 + sl * G + g) * 2] - M);
        L = fmaf(p.pfx_ml[(a0 + sl * G + g) * 2 + 1], f, L);
        O = fmaf(p.pfx_o[(a0 + sl * G + g) * 128 + d], f, O);
    }
    for (int sl = 0; sl < active; ++sl) {
        const float f = __expf(p.part_ml[(b0 + sl * G + g) * 2] - M);
        L = fmaf(p.part_ml[(b0 + sl * G + g) * 2 + 1], f, L);
        O = fmaf(p.part_o[(b0 + sl * G + g) * 128 + d], f, O);
    }
    p.o[(int64_t)row * p.o_row_stride + h * 128 + d] = f2bf(O / L);
}
template <int G>
static int launch_bdec_prefix_g(const BSharedArgs& sh, const BAttnArgs& a, int rows, hipStream_t s) {
    VILA_TRY((launch_bdec_shared_g<G, true>(sh, s)));
    const size_t lds = (size_t)(16 * G * 128 + 16 * G * 2) * 4 + 16 * 272;
    static bool attr = false;
    if (!attr) {
        VILA_HIP(hipFuncSetAttribute((const void*)bdec_attn_walk_kernel<G, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    hipLaunchKernelGGL((bdec_attn_walk_kernel<G, true>), dim3(a.nkv, a.nsl, rows), dim3(1024), lds, s, a);
    VILA_LAUNCH_CHECK();
    hipLaunchKernelGGL(bdec_attn_prefix_merge_kernel, dim3(a.nq, rows), dim3(128), 0, s, a, G);
    VILA_LAUNCH_CHECK();
    return 0;
}
// the two partial sets, each two separately aligned arrays: the private phase's at the batched step's slot count, the prefix phase's at the verify form's
size_t bprefix_attn_workspace_bytes(int rows, int nq, int max_ctx) {
    return bdecode_attn_workspace_bytes(rows, nq, max_ctx) + bverify_attn_workspace_bytes(rows, nq, max_ctx);
}
// the launches alone, on partials the caller has laid out for bdec_attn_form(max_ctx).nsl private and bverify_attn_slices(max_ctx) prefix slices
int bprefix_attn_launch(const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, int prefix_slot, const int32_t* shared_len,
                        const int32_t* uses, const int32_t* pos, bf16_t* o, int64_t ldo, int rows, int nq, int nkv, int max_ctx, float scale, float* part_o,
                        float* part_ml, float* pfx_o, float* pfx_ml, hipStream_t s) {
    BSharedArgs sh{};
    sh.q = q; sh.o = o; sh.kslot = kcache + (int64_t)prefix_slot * slot_stride; sh.vslot = vcache + (int64_t)prefix_slot * slot_stride; sh.pos = shared_len;
    sh.part_o = pfx_o; sh.part_ml = pfx_ml; sh.n = rows; sh.nq = nq; sh.nkv = nkv; sh.max_ctx = max_ctx; sh.nsl = bverify_attn_slices(max_ctx);
    sh.ldq = ldq; sh.ldo = ldo; sh.scale = scale;
    BAttnArgs a{};
    a.q = q; a.o = o; a.kcache = kcache; a.vcache = vcache; a.pos = pos; a.part_o = part_o; a.part_ml = part_ml;
    a.nq = nq; a.nkv = nkv; a.max_ctx = max_ctx; a.nsl = bdec_attn_form(max_ctx).nsl; a.row_stride = ldq; a.o_row_stride = ldo; a.slot_stride = slot_stride;
    a.scale = scale; a.shared_len = shared_len; a.uses = uses; a.pfx_o = pfx_o; a.pfx_ml = pfx_ml; a.psl = sh.nsl;
    switch (nq / nkv) {
        case 1: return launch_bdec_prefix_g<1>(sh, a, rows, s);
        case 2: return launch_bdec_prefix_g<2>(sh, a, rows, s);
        case 4: return launch_bdec_prefix_g<4>(sh, a, rows, s);
        case 7: return launch_bdec_prefix_g<7>(sh, a, rows, s);
        case 8: return launch_bdec_prefix_g<8>(sh, a, rows, s);
        default: break;
    }
    VILA_REQUIRE(false, "attn_decode_batch_prefix: GQA groups of 1, 2, 4, 7 or 8 query heads per kv head (got %d)", nq / nkv);
    return -1;
}
// shared_len_host: S where the host knows it (refused unless a multiple of 256 inside the slot), -1 where it does not
int bprefix_attn(const bf16_t* q, int64_t ldq, const bf16_t* kcache, const bf16_t* vcache, int64_t slot_stride, int n_slots, int prefix_slot,
                 const int32_t* shared_len, int shared_len_host, const int32_t* uses, const int32_t* pos, bf16_t* o, int64_t ldo, int rows, int nq, int nkv,
                 int max_ctx, float scale, void* workspace, size_t workspace_bytes, hipStream_t s) {
    VILA_REQUIRE(q && kcache && vcache && shared_len && uses && pos && o && workspace, "attn_decode_batch_prefix: NULL argument");
    VILA_REQUIRE(rows >= 1 && rows <= 16 && nkv >= 1 && nq % nkv == 0 && bdec_group_ok(nq / nkv),
                 "attn_decode_batch_prefix: 1..16 rows and a GQA group of 1, 2, 4, 7 or 8 query heads per kv head (got %d rows, %d / %d heads)", rows, nq, nkv);
    VILA_REQUIRE(max_ctx >= 1 && max_ctx <= BDEC_MAX_CTX, "attn_decode_batch_prefix: caches of 1..%d positions (got %d)", BDEC_MAX_CTX, max_ctx);
    VILA_REQUIRE(n_slots > rows && prefix_slot >= rows && prefix_slot < n_slots,
                 "attn_decode_batch_prefix: the prefix slot (%d) is a slot of the cache (%d slots) behind the %d rows' own", prefix_slot, n_slots, rows);
    VILA_REQUIRE(shared_len_host == -1 || (shared_len_host >= 0 && shared_len_host <= max_ctx && shared_len_host % 256 == 0),
                 "attn_decode_batch_prefix: the shared length is a multiple of 256 within the slot (got %d of %d)", shared_len_host, max_ctx);
    VILA_REQUIRE(ldq % 8 == 0 && ldq >= (int64_t)nq * 128 && ldo >= (int64_t)nq * 128 && (uintptr_t)q % 16 == 0 && (uintptr_t)kcache % 16 == 0 &&
                 (uintptr_t)vcache % 16 == 0 && slot_stride % 8 == 0 && slot_stride >= (int64_t)nkv * max_ctx * 128,
                 "attn_decode_batch_prefix: head_dim 128 rows, 16-byte aligned, slots of [kv_heads][max_ctx][128]");
    VILA_REQUIRE(workspace_bytes >= bprefix_attn_workspace_bytes(rows, nq, max_ctx), "attn_decode_batch_prefix: workspace too small");
    const size_t nsl = (size_t)bdec_attn_form(max_ctx).nsl, psl = (size_t)bverify_attn_slices(max_ctx);
    char* w = (char*)workspace;
    float* part_o = (float*)w;
    float* part_ml = (float*)(w + align_up((size_t)rows * nq * nsl * 128 * 4, 256));
    w += bdecode_attn_workspace_bytes(rows, nq, max_ctx);
    float* pfx_o = (float*)w;
    float* pfx_ml = (float*)(w + align_up((size_t)rows * nq * psl * 128 * 4, 256));
    return bprefix_attn_launch(q, ldq, kcache, vcache, slot_stride, prefix_slot, shared_len, uses, pos, o, ldo, rows, nq, nkv, max_ctx, scale, part_o, part_ml,
                               pfx_o, pfx_ml, s);
}

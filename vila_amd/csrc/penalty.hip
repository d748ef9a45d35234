// Repetition, presence and frequency penalties in front of the token choice: the first element of HF's logits-processor chain, which runs before
// temperature -> top-k -> top-p (sample.hip's header has that order).  The decode steps write raw fp32 logits and then pick; this launch sits between
// the two, on the device, so a penalised step still replays from one hipGraph.
//
// State: counts[row][vocab] uint16 = how often the request of that row has generated each id (zero when it starts, saturating at 65535; the prompt
// is not counted: the reference passes inputs_embeds only, and HF's input_ids is then empty at the first step).  Per (row, index i), in this order:
//   bump        counts[row][token[row]] += 1 for the token the step consumes (the one chosen a step earlier), by the thread that owns that index,
//               before the count is used; an id outside 0 .. vocab - 1 bumps nothing.  At step k the table is HF's input_ids.
//   repetition  c > 0:  y = x < 0 ? x * rep : x / rep          (HF RepetitionPenaltyLogitsProcessor; -0.0 takes the division and stays -0.0)
//   frequency   y = y - freq * float(c)                         (OpenAI's definition, vLLM's order)
//   presence    c > 0:  y = y - pres
// Every operation is ONE correctly rounded fp32 operation (__fmul_rn / __fdiv_rn / __fsub_rn, nothing contracted into an FMA), so y is bit for bit
// the torch expression on the CPU, and rep = 1, pres = freq = 0 reproduce x bit for bit (x / 1, x * 1, x - 0 * c, x - 0).
// The launch also does the greedy pick's first stage: one (max, first index) pair of y per (slice, row), pairs[row * n_slices + slice] — with
// PICK_SLICES slices the layout bdec_pick1_kernel writes, so bdec_pick2_kernel merges them.  The rep / pres / freq of a row are read from device
// arrays: one captured graph serves any mix of rows and values.
// Grid (n_slices, n) x 256 threads.  A slice is a multiple of 4 indices, so that where the row bases and strides allow it (16-byte logits and output
// rows, 8-byte count rows) a thread moves 4 logits, 4 counts and 4 outputs per access; the end of a row that is no multiple of 4 and rows that are not
// aligned take the scalar path.  Nothing at or beyond `vocab` is read or written.
#include "kernels.h"

__device__ __forceinline__ float pen_apply(float x, uint32_t c, float rep, float pres, float freq) {
    float y = x;
    if (c > 0u) y = x < 0.f ? __fmul_rn(x, rep) : __fdiv_rn(x, rep);
    y = __fsub_rn(y, __fmul_rn(freq, (float)c));
    if (c > 0u) y = __fsub_rn(y, pres);
    return y;
}
__device__ __forceinline__ uint32_t pen_bump(uint32_t c) { return c < 65535u ? c + 1u : 65535u; }

template <bool VEC>
__global__ __launch_bounds__(256) void penalize_kernel(const float* __restrict__ logits, int64_t ld, int V, const float* __restrict__ repetition,
                                                       const float* __restrict__ presence, const float* __restrict__ frequency, uint16_t* __restrict__ counts,
                                                       int64_t ld_counts, const int64_t* __restrict__ token, float* __restrict__ out, int64_t ld_out,
                                                       int n_slices, float* __restrict__ pv, int* __restrict__ pi) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int per = (((V + n_slices - 1) / n_slices) + 3) & ~3;
    const int lo = sl * per < V ? sl * per : V, hi = lo + per < V ? lo + per : V;
    const float rep = repetition[row], pres = presence[row], freq = frequency[row];
    const int64_t t64 = token != nullptr ? token[row] : (int64_t)-1;
    const int tok = (t64 >= 0 && t64 < (int64_t)V) ? (int)t64 : -1;
    const float* lr = logits + (int64_t)row * ld;
    uint16_t* cr = counts + (int64_t)row * ld_counts;
    float* yr = out + (int64_t)row * ld_out;
    float best = -INFINITY; int bi = 0x7fffffff;
    // one index: the owner of `tok` bumps its count in the register it computes from and writes the new count back
    auto one = [&](int i) {
        uint32_t c = cr[i];
        if (i == tok) { c = pen_bump(c); cr[i] = (uint16_t)c; }
        const float y = pen_apply(lr[i], c, rep, pres, freq);
        yr[i] = y;
        if (y > best || (y == best && i < bi)) { best = y; bi = i; }
    };
    if constexpr (VEC) {
        for (int i = lo + 4 * tid; i < hi; i += 4 * 256) {
            if (i + 4 <= hi) {
                const f32x4 x = *(const f32x4*)(lr + i);
                const uint2 cw = *(const uint2*)(cr + i);
                uint32_t c[4] = {cw.x & 0xffffu, cw.x >> 16, cw.y & 0xffffu, cw.y >> 16};
                if (tok >= i && tok < i + 4) { const int j = tok - i; c[j] = pen_bump(c[j]); cr[tok] = (uint16_t)c[j]; }
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] = pen_apply(x[j], c[j], rep, pres, freq);
                    if (y[j] > best || (y[j] == best && i + j < bi)) { best = y[j]; bi = i + j; }
                }
                *(f32x4*)(yr + i) = y;
            } else {
                for (int j = i; j < hi; ++j) one(j);
            }
        }
    } else {
        for (int i = lo + tid; i < hi; i += 256) one(i);
    }
    if (pv == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, 64); const int i2 = __shfl_xor(bi, o, 64);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        pv[row * n_slices + sl] = best; pi[row * n_slices + sl] = bi;
    }
}

int launch_penalize(const float* logits, int64_t ld, int n, int vocab, const Penalties& p, const int64_t* token, float* out, int64_t ld_out, int n_slices,
                    float* pick_v, int* pick_i, hipStream_t s) {
    VILA_REQUIRE(logits != nullptr && out != nullptr && p.repetition != nullptr && p.presence != nullptr && p.frequency != nullptr && p.counts != nullptr,
                 "logits_penalize: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 65535 && vocab >= 1, "logits_penalize: 1..65535 rows of a non-empty vocabulary (got %d x %d)", n, vocab);
    VILA_REQUIRE(ld >= vocab && ld_out >= vocab && p.ld_counts >= vocab, "logits_penalize: a row stride (%lld, %lld, %lld) is below the vocabulary %d",
                 (long long)ld, (long long)ld_out, (long long)p.ld_counts, vocab);
    VILA_REQUIRE((pick_v == nullptr) == (pick_i == nullptr) && n_slices >= 1 && n_slices <= 65535, "logits_penalize: the pairs need both arrays and 1..65535 slices");
    const bool vec = (uintptr_t)logits % 16 == 0 && ld % 4 == 0 && (uintptr_t)out % 16 == 0 && ld_out % 4 == 0 && (uintptr_t)p.counts % 8 == 0 && p.ld_counts % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(penalize_kernel<true>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, p.repetition, p.presence, p.frequency, p.counts, p.ld_counts,
                           token, out, ld_out, n_slices, pick_v, pick_i);
    else
        hipLaunchKernelGGL(penalize_kernel<false>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, p.repetition, p.presence, p.frequency, p.counts, p.ld_counts,
                           token, out, ld_out, n_slices, pick_v, pick_i);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ---- the verify form (speculative decoding, decode_batch.hip bverify_step) --------------------------------------------------------------------
// n rows of ONE sequence: row i consumes token[i] behind token[0 .. i - 1], so it is penalised with the counts the session drafting nothing would hold
// at that step: c_i(v) = min(65535, counts[v] + #{j <= i : token[j] == v}) — the saturating sum, which equals the sequential saturating bumps.  ONE
// count row and ONE entry per parameter array serve every row, and the launch only READS the table: what the step accepts is committed behind the
// accept (verify_commit_kernel).  Per block, thread 0 stages the ids of token[0 .. row] that fall into the block's slice in LDS (at most 16; an id
// outside 0 .. vocab - 1 lies in no slice and counts nothing); a slice without one — nearly all of them — adds nothing to the loaded counts.
// Same grid, vector path, scalar tail and (max, first index) pairs as penalize_kernel.
template <bool VEC>
__global__ __launch_bounds__(256) void penalize_verify_kernel(const float* __restrict__ logits, int64_t ld, int V, const float* __restrict__ repetition,
                                                              const float* __restrict__ presence, const float* __restrict__ frequency,
                                                              const uint16_t* __restrict__ counts, const int64_t* __restrict__ token, float* __restrict__ out,
                                                              int64_t ld_out, int n_slices, float* __restrict__ pv, int* __restrict__ pi) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int tk[PEN_VERIFY_MAX_ROWS];
    __shared__ int ntk;
    const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int per = (((V + n_slices - 1) / n_slices) + 3) & ~3;
    const int lo = sl * per < V ? sl * per : V, hi = lo + per < V ? lo + per : V;
    if (tid == 0) {
        int c = 0;
        for (int j = 0; j <= row && j < PEN_VERIFY_MAX_ROWS; ++j) {
            const int64_t t = token[j];
            if (t >= (int64_t)lo && t < (int64_t)hi) tk[c++] = (int)t;
        }
        ntk = c;
    }
    __syncthreads();
    const int nt = ntk;
    const float rep = repetition[0], pres = presence[0], freq = frequency[0];
    const float* lr = logits + (int64_t)row * ld;
    float* yr = out + (int64_t)row * ld_out;
    float best = -INFINITY; int bi = 0x7fffffff;
    auto sat = [](uint32_t c) { return c < 65535u ? c : 65535u; };
    auto one = [&](int i) {
        uint32_t c = counts[i];
        for (int j = 0; j < nt; ++j) c += tk[j] == i ? 1u : 0u;
        const float y = pen_apply(lr[i], sat(c), rep, pres, freq);
        yr[i] = y;
        if (y > best || (y == best && i < bi)) { best = y; bi = i; }
    };
    if constexpr (VEC) {
        for (int i = lo + 4 * tid; i < hi; i += 4 * 256) {
            if (i + 4 <= hi) {
                const f32x4 x = *(const f32x4*)(lr + i);
                const uint2 cw = *(const uint2*)(counts + i);
                uint32_t c[4] = {cw.x & 0xffffu, cw.x >> 16, cw.y & 0xffffu, cw.y >> 16};
                for (int j = 0; j < nt; ++j) {
                    const int t = tk[j];
#pragma unroll
                    for (int q = 0; q < 4; ++q) c[q] += t == i + q ? 1u : 0u;
                }
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] = pen_apply(x[j], sat(c[j]), rep, pres, freq);
                    if (y[j] > best || (y[j] == best && i + j < bi)) { best = y[j]; bi = i + j; }
                }
                *(f32x4*)(yr + i) = y;
            } else {
                for (int j = i; j < hi; ++j) one(j);
            }
        }
    } else {
        for (int i = lo + tid; i < hi; i += 256) one(i);
    }
    if (pv == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, 64); const int i2 = __shfl_xor(bi, o, 64);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        pv[row * n_slices + sl] = best; pi[row * n_slices + sl] = bi;
    }
}

int launch_penalize_verify(const float* logits, int64_t ld, int n, int vocab, const Penalties& p, const int64_t* token, float* out, int64_t ld_out, int n_slices,
                           float* pick_v, int* pick_i, hipStream_t s) {
    VILA_REQUIRE(logits != nullptr && out != nullptr && token != nullptr && p.repetition != nullptr && p.presence != nullptr && p.frequency != nullptr &&
                 p.counts != nullptr, "logits_penalize_verify: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= PEN_VERIFY_MAX_ROWS && vocab >= 1, "logits_penalize_verify: 1..%d rows of a non-empty vocabulary (got %d x %d)",
                 PEN_VERIFY_MAX_ROWS, n, vocab);
    VILA_REQUIRE(ld >= vocab && ld_out >= vocab && p.ld_counts >= vocab, "logits_penalize_verify: a row stride (%lld, %lld, %lld) is below the vocabulary %d",
                 (long long)ld, (long long)ld_out, (long long)p.ld_counts, vocab);
    VILA_REQUIRE((pick_v == nullptr) == (pick_i == nullptr) && n_slices >= 1 && n_slices <= 65535,
                 "logits_penalize_verify: the pairs need both arrays and 1..65535 slices");
    const bool vec = (uintptr_t)logits % 16 == 0 && ld % 4 == 0 && (uintptr_t)out % 16 == 0 && ld_out % 4 == 0 && (uintptr_t)p.counts % 8 == 0;
    if (vec)
        hipLaunchKernelGGL(penalize_verify_kernel<true>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, p.repetition, p.presence, p.frequency,
                           (const uint16_t*)p.counts, token, out, ld_out, n_slices, pick_v, pick_i);
    else
        hipLaunchKernelGGL(penalize_verify_kernel<false>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, p.repetition, p.presence, p.frequency,
                           (const uint16_t*)p.counts, token, out, ld_out, n_slices, pick_v, pick_i);
    VILA_LAUNCH_CHECK();
    return 0;
}

// The commit behind the accept, by ONE thread: the step accepted m = *n_accept drafts, so it consumed consumed[0 .. m] (the copy of token[] taken before
// the accept overwrote token[0]).  Each gets one saturating bump of the count row, in order (one thread: a repeated id cannot race), and the automaton
// moves to states[m], the chain's state behind consumed[m].  Nothing of the rows behind m — rejected drafts and padding — reaches the table or the state.
// counts / state nullable: one launch serves penalties, an automaton or both.
__global__ __launch_bounds__(64) void verify_commit_kernel(uint16_t* __restrict__ counts, int V, int32_t* __restrict__ state, const int64_t* __restrict__ consumed,
                                                           const int32_t* __restrict__ states, const int32_t* __restrict__ n_accept, int n) {
    if (threadIdx.x != 0) return;
    int m = *n_accept;
    m = m < 0 ? 0 : (m > n - 1 ? n - 1 : m);
    if (counts != nullptr) {
        for (int j = 0; j <= m; ++j) {
            const int64_t t = consumed[j];
            if (t >= 0 && t < (int64_t)V) counts[t] = (uint16_t)pen_bump(counts[t]);
        }
    }
    if (state != nullptr) *state = states[m];
}
int launch_verify_commit(uint16_t* counts, int vocab, int32_t* state, const int64_t* consumed, const int32_t* states, const int32_t* n_accept, int n,
                         hipStream_t s) {
    VILA_REQUIRE(counts != nullptr || state != nullptr, "verify_commit: neither a count row nor an automaton state");
    VILA_REQUIRE(n_accept != nullptr && n >= 1 && n <= PEN_VERIFY_MAX_ROWS && vocab >= 1, "verify_commit: 1..%d rows, a vocabulary and the accepted count (got %d, %d)",
                 PEN_VERIFY_MAX_ROWS, n, vocab);
    VILA_REQUIRE((counts == nullptr || consumed != nullptr) && (state == nullptr || states != nullptr),
                 "verify_commit: the counts need the consumed tokens, the state needs the chain's states");
    hipLaunchKernelGGL(verify_commit_kernel, dim3(1), dim3(64), 0, s, counts, vocab, state, consumed, states, n_accept, n);
    VILA_LAUNCH_CHECK();
    return 0;
}

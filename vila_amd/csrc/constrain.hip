// Structured output: a token-level automaton per row in front of the token choice.  The decode steps write raw fp32 logits and then pick; like the
// penalty launch (penalty.hip) this one sits between the two, on the device, so a constrained step still replays from one hipGraph.  It runs BEHIND the
// penalties (HF's order: a caller's logits_processor follows the built-in processors and precedes temperature -> top-k -> top-p).
//
// Row r carries a deterministic automaton over token CLASSES (vila_amd/constrain.py compiles it): cls[r][id] = the class of every token id,
// next[r] = its table, row-major [n_states][C] with C = n_classes[r], an entry < 0 = that class is not allowed in that state; state[r] = its current
// state, -1 = the row is unconstrained.  Two launches:
//   advance  ONE block, ahead of the mask: s = state[r] >= 0 and the consumed token t = token[r] in 0 .. vocab - 1 -> s2 = next[r][s * C + cls[r][t]];
//            s2 >= 0 replaces the state, anything else leaves it.  (The step counts the token it consumes, the penalties' convention; the eager
//            first-token call passes no token and masks from the start state.)  A launch of its own, so that no block of the mask launch reads a word
//            another block of its launch writes.
//   mask     grid (n_slices, n) x 256: y[i] = next[r][state * C + cls[r][i]] >= 0 ? x[i] : -inf for i < vocab; an unconstrained row copies x bit for
//            bit.  The state's table row (at most CON_MAX_CLASSES int16, 8 KB) is loaded into LDS once per block.  out may alias logits (every index
//            is read and written by the same thread).  The launch also does the greedy pick's first stage, like penalize_kernel: one (max, first
//            index) pair of y per (slice, row), pairs[row * n_slices + slice].  An all -inf slice reports its first index, so an all -inf row merges
//            to index 0.
// The kernel cannot validate device contents; it only keeps its own reads in bounds: a class >= C or a table row beyond ld_next counts as not allowed.
// A slice is a multiple of 4 indices; where the row bases and strides allow it (16-byte logits and output rows, 8-byte class rows) a thread moves 4
// logits, 4 classes and 4 outputs per access; the end of a row that is no multiple of 4 and rows that are not aligned take the scalar path.  Nothing at
// or beyond `vocab` is read or written.
#include "kernels.h"

__global__ __launch_bounds__(256) void constrain_advance_kernel(int32_t* __restrict__ state, const uint16_t* __restrict__ cls, int64_t ld_cls,
                                                                const int16_t* __restrict__ next, int64_t ld_next, const int32_t* __restrict__ n_classes,
                                                                const int64_t* __restrict__ token, int n, int V) {
    for (int r = threadIdx.x; r < n; r += 256) {
        const int s = state[r];
        const int64_t t = token[r];
        if (s < 0 || t < 0 || t >= (int64_t)V) continue;
        const int C = n_classes[r];
        if (C < 1 || C > CON_MAX_CLASSES || ((int64_t)s + 1) * C > ld_next) continue;
        const int c = cls[(int64_t)r * ld_cls + t];
        if (c >= C) continue;
        const int s2 = next[(int64_t)r * ld_next + (int64_t)s * C + c];
        if (s2 >= 0) state[r] = s2;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void constrain_mask_kernel(const float* logits, int64_t ld, int V, const int32_t* __restrict__ state,
                                                             const uint16_t* __restrict__ cls, int64_t ld_cls, const int16_t* __restrict__ next,
                                                             int64_t ld_next, const int32_t* __restrict__ n_classes, float* out, int64_t ld_out,
                                                             int n_slices, float* __restrict__ pv, int* __restrict__ pi, int one_auto) {
    __shared__ int16_t trow[CON_MAX_CLASSES];
    __shared__ float sv[4];
    __shared__ int si[4];
    const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int per = (((V + n_slices - 1) / n_slices) + 3) & ~3;
    const int lo = sl * per < V ? sl * per : V, hi = lo + per < V ? lo + per : V;
    const int s = state[row];                                       // block-uniform
    const int arow = one_auto ? 0 : row;                            // the verify form: every row is a state of automaton 0 (constrain_chain_kernel)
    const bool free_row = s < 0;
    int C = 0;
    if (!free_row) {
        C = n_classes[arow];
        if (C < 1 || C > CON_MAX_CLASSES || ((int64_t)s + 1) * C > ld_next) C = 0;          // nothing allowed: no read outside the row's table
        const int16_t* tr = next + (int64_t)arow * ld_next + (int64_t)s * C;
        for (int c = tid; c < C; c += 256) trow[c] = tr[c];
        __syncthreads();
    }
    const float* lr = logits + (int64_t)row * ld;
    const uint16_t* cr = cls + (int64_t)arow * ld_cls;
    float* yr = out + (int64_t)row * ld_out;
    float best = -INFINITY; int bi = 0x7fffffff;
    auto ok = [&](uint32_t c) { return free_row || ((int)c < C && trow[c] >= 0); };
    auto one = [&](int i) {
        const float y = ok(free_row ? 0u : (uint32_t)cr[i]) ? lr[i] : -INFINITY;
        yr[i] = y;
        if (y > best || (y == best && i < bi)) { best = y; bi = i; }
    };
    if constexpr (VEC) {
        for (int i = lo + 4 * tid; i < hi; i += 4 * 256) {
            if (i + 4 <= hi) {
                const f32x4 x = *(const f32x4*)(lr + i);
                uint2 cw = make_uint2(0u, 0u);
                if (!free_row) cw = *(const uint2*)(cr + i);
                const uint32_t c[4] = {cw.x & 0xffffu, cw.x >> 16, cw.y & 0xffffu, cw.y >> 16};
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] = ok(c[j]) ? x[j] : -INFINITY;
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

int launch_constrain(const float* logits, int64_t ld, int n, int vocab, const Constraints& c, const int64_t* token, float* out, int64_t ld_out, int n_slices,
                     float* pick_v, int* pick_i, hipStream_t s) {
    VILA_REQUIRE(logits != nullptr && out != nullptr && c.state != nullptr && c.cls != nullptr && c.next != nullptr && c.n_classes != nullptr,
                 "logits_constrain: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 65535 && vocab >= 1, "logits_constrain: 1..65535 rows of a non-empty vocabulary (got %d x %d)", n, vocab);
    VILA_REQUIRE(ld >= vocab && ld_out >= vocab && c.ld_cls >= vocab, "logits_constrain: a row stride (%lld, %lld, %lld) is below the vocabulary %d",
                 (long long)ld, (long long)ld_out, (long long)c.ld_cls, vocab);
    VILA_REQUIRE(c.ld_next >= 1, "logits_constrain: the table rows are %lld entries apart", (long long)c.ld_next);
    VILA_REQUIRE((pick_v == nullptr) == (pick_i == nullptr) && n_slices >= 1 && n_slices <= 65535, "logits_constrain: the pairs need both arrays and 1..65535 slices");
    if (token != nullptr) {
        hipLaunchKernelGGL(constrain_advance_kernel, dim3(1), dim3(256), 0, s, c.state, c.cls, c.ld_cls, c.next, c.ld_next, c.n_classes, token, n, vocab);
        VILA_LAUNCH_CHECK();
    }
    const bool vec = (uintptr_t)logits % 16 == 0 && ld % 4 == 0 && (uintptr_t)out % 16 == 0 && ld_out % 4 == 0 && (uintptr_t)c.cls % 8 == 0 && c.ld_cls % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(constrain_mask_kernel<true>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, (const int32_t*)c.state, c.cls, c.ld_cls, c.next,
                           c.ld_next, c.n_classes, out, ld_out, n_slices, pick_v, pick_i, 0);
    else
        hipLaunchKernelGGL(constrain_mask_kernel<false>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, (const int32_t*)c.state, c.cls, c.ld_cls, c.next,
                           c.ld_next, c.n_classes, out, ld_out, n_slices, pick_v, pick_i, 0);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ---- the verify form (speculative decoding, decode_batch.hip bverify_step) --------------------------------------------------------------------
// n rows of ONE sequence under ONE automaton: row i consumes token[i] behind token[0 .. i - 1], so it is masked from s_i with s_0 = adv(state, token[0]),
// s_i = adv(s_{i-1}, token[i]) — adv being constrain_advance_kernel's rule word for word.  The chain is at most 16 dependent lookups by ONE thread; it
// lands in states_out and leaves `state` alone: what the step accepts is committed behind the accept (penalty.hip verify_commit_kernel).  The other
// lanes of the wave keep the consumed tokens (consumed[i] = token[i], nullable), which the accept is about to overwrite.  state NULL: the copy only.
// The mask kernel then runs with the per-row states of the chain and automaton 0's classes and table for every row (one_auto).
__global__ __launch_bounds__(64) void constrain_chain_kernel(const int32_t* __restrict__ state, const uint16_t* __restrict__ cls, const int16_t* __restrict__ next,
                                                             int64_t ld_next, const int32_t* __restrict__ n_classes, const int64_t* __restrict__ token, int n, int V,
                                                             int32_t* __restrict__ states_out, int64_t* __restrict__ consumed) {
    const int tid = threadIdx.x;
    if (consumed != nullptr && tid < n) consumed[tid] = token[tid];
    if (tid != 0 || state == nullptr) return;
    int s = state[0];
    const int C = n_classes[0];
    for (int i = 0; i < n; ++i) {
        const int64_t t = token[i];
        if (s >= 0 && t >= 0 && t < (int64_t)V && C >= 1 && C <= CON_MAX_CLASSES && ((int64_t)s + 1) * C <= ld_next) {
            const int c = cls[t];
            if (c < C) {
                const int s2 = next[(int64_t)s * C + c];
                if (s2 >= 0) s = s2;
            }
        }
        states_out[i] = s;
    }
}
int launch_verify_chain(const Constraints* c, const int64_t* token, int n, int vocab, int32_t* states_out, int64_t* consumed, hipStream_t s) {
    VILA_REQUIRE(token != nullptr && n >= 1 && n <= 64 && vocab >= 1, "constrain_verify: 1..64 rows of one sequence and their tokens (got %d)", n);
    VILA_REQUIRE(c != nullptr || consumed != nullptr, "constrain_verify: neither an automaton nor a place for the consumed tokens");
    VILA_REQUIRE(c == nullptr || (c->state != nullptr && c->cls != nullptr && c->next != nullptr && c->n_classes != nullptr && states_out != nullptr &&
                                  c->ld_cls >= vocab && c->ld_next >= 1), "constrain_verify: NULL argument or a class row below the vocabulary");
    if (c != nullptr)
        hipLaunchKernelGGL(constrain_chain_kernel, dim3(1), dim3(64), 0, s, (const int32_t*)c->state, c->cls, c->next, c->ld_next, c->n_classes, token, n, vocab,
                           states_out, consumed);
    else
        hipLaunchKernelGGL(constrain_chain_kernel, dim3(1), dim3(64), 0, s, (const int32_t*)nullptr, (const uint16_t*)nullptr, (const int16_t*)nullptr, (int64_t)0,
                           (const int32_t*)nullptr, token, n, vocab, (int32_t*)nullptr, consumed);
    VILA_LAUNCH_CHECK();
    return 0;
}
int launch_constrain_rows(const float* logits, int64_t ld, int n, int vocab, const Constraints& c, const int32_t* states, float* out, int64_t ld_out, int n_slices,
                          float* pick_v, int* pick_i, hipStream_t s) {
    VILA_REQUIRE(logits != nullptr && out != nullptr && states != nullptr && c.cls != nullptr && c.next != nullptr && c.n_classes != nullptr,
                 "constrain_verify: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 64 && vocab >= 1, "constrain_verify: 1..64 rows of a non-empty vocabulary (got %d x %d)", n, vocab);
    VILA_REQUIRE(ld >= vocab && ld_out >= vocab && c.ld_cls >= vocab, "constrain_verify: a row stride (%lld, %lld, %lld) is below the vocabulary %d",
                 (long long)ld, (long long)ld_out, (long long)c.ld_cls, vocab);
    VILA_REQUIRE(c.ld_next >= 1, "constrain_verify: the table holds %lld entries", (long long)c.ld_next);
    VILA_REQUIRE((pick_v == nullptr) == (pick_i == nullptr) && n_slices >= 1 && n_slices <= 65535, "constrain_verify: the pairs need both arrays and 1..65535 slices");
    const bool vec = (uintptr_t)logits % 16 == 0 && ld % 4 == 0 && (uintptr_t)out % 16 == 0 && ld_out % 4 == 0 && (uintptr_t)c.cls % 8 == 0;
    if (vec)
        hipLaunchKernelGGL(constrain_mask_kernel<true>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, states, c.cls, c.ld_cls, c.next, c.ld_next, c.n_classes,
                           out, ld_out, n_slices, pick_v, pick_i, 1);
    else
        hipLaunchKernelGGL(constrain_mask_kernel<false>, dim3(n_slices, n), dim3(256), 0, s, logits, ld, vocab, states, c.cls, c.ld_cls, c.next, c.ld_next, c.n_classes,
                           out, ld_out, n_slices, pick_v, pick_i, 1);
    VILA_LAUNCH_CHECK();
    return 0;
}

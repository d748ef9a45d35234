// Log-probabilities of the chosen token and of the 20 most likely alternatives, from the RAW fp32 logits of a decode step (or of any rows of logits):
// the `logprobs` / `top_logprobs` of an OpenAI-style endpoint, HF's `compute_transition_scores`.  For a row x[0 .. V-1]:
//   M = max x,  lse = M + log(sum_i exp(x_i - M)),  logprob(t) = x_t - lse          (all fp32; an -inf entry contributes 0)
// and the alternatives are the largest raw logits in descending order, ties towards the LOWER index: the order of smp_key (kernels.h), decided by
// comparing the keys only, so the ids are exact.  The numbers describe the model's own distribution: temperature, top-k, top-p and penalties do not
// enter, whatever the session's pick does.
// Two launches whatever the number of rows, every reduction in a fixed order and no floating-point atomic: the same bits on every run, and a row's
// bits depend neither on the other rows of the launch nor on where the row lies (element j of a slice belongs to the same thread and register
// whether the row is read with 16-byte or with 4-byte loads).
//   stage 1  grid (slices, rows) x 256 threads.  A row is cut into lp_slices(V) <= LP_MAX_SLICES contiguous slices of lp_slice_width(V) logits (a
//            multiple of 4, at least 1024).  A block walks its slice in chunks of LP_CHUNK logits held in registers (16 per thread: thread t owns
//            elements 1024 q + 4 t .. + 3 of the chunk, q = 0 .. 3), read ONCE: f32x4 loads where the chunk starts on a 16-byte boundary, scalar loads
//            otherwise and for the group that crosses the end of the row.  Per chunk it selects the 20 largest keys of (chunk + best so far)
//            (lp_top20 below) — the first of which holds the largest value so far — and folds the chunk into a running (max, sum exp(x - max))
//            pair: per thread in register order, per wave by an xor butterfly, the four waves in order, the chunks in order.
//   stage 2  one block per row merges the slices in index order, M = max m_s, L = sum_s sum_s exp(m_s - M), lse = M + log L, selects the 20
//            largest of the <= 48 x 20 candidate keys with the same lp_top20, reads the chosen token's logit and writes the row's record.
// lp_top20: every thread holds M keys (distinct, or 0 = none).  The 20 largest of the block lie in the 20 threads whose own largest key (head) is
// largest: T = the head of rank 19, found by counting for every head the heads above it; the keys >= T (at most 20 x M) go to a candidate list,
// and a candidate whose count of larger candidates is r < 20 is the r-th largest.  Ranks are counted by comparisons, so the result does not depend
// on the order in which the (integer, LDS) atomic hands out the places of the list.  Five barriers instead of a sort or 20 block-wide maxima.
// Records: row r writes record rec[r] + rec_bias (rec NULL: rec_bias) of token_logprob [n][max_rec] and top_logprob / top_id [n][max_rec][20]; an
// index outside 0 .. max_rec - 1 writes NOTHING (an idle row of a batch steps past its buffers).  Places from top_n on, and places a vocabulary
// below 20 cannot fill, hold id -1 / -inf.  A token outside 0 .. V - 1 gives NaN for the chosen logprob and disturbs nothing else.
// one_seq (the verify step): the rows are steps of ONE sequence, so every row writes output row 0 — record rec[r] of token_logprob [max_rec] etc.
// Nothing at or beyond `vocab` within a row is read; nothing outside the records and the workspace is written.
#include "kernels.h"

#define LP_MAX_SLICES 48            // x LP_TOP = 960 candidates in stage 2: four keys per thread
#define LP_CHUNK 4096               // logits a block holds in registers at a time: 16 per thread

int logprob_slice_width(int vocab) {
    const int64_t per = ((((int64_t)vocab + LP_MAX_SLICES - 1) / LP_MAX_SLICES) + 3) & ~(int64_t)3;
    return per < 1024 ? 1024 : (int)per;
}
static inline int lp_slices(int vocab) { const int per = logprob_slice_width(vocab); return (int)(((int64_t)vocab + per - 1) / per); }
// per row: the candidate keys [LP_MAX_SLICES][LP_TOP], then the (max, sum) pairs [LP_MAX_SLICES][2]
#define LP_ROW_KEYS (LP_MAX_SLICES * LP_TOP)
size_t logprob_workspace_bytes(int n) { return (size_t)(n > 0 ? n : 0) * (LP_ROW_KEYS * sizeof(uint64_t) + LP_MAX_SLICES * 2 * sizeof(float)) + 256; }

#define LP_MAX_M 17                 // keys a thread brings to lp_top20 at most: the 16 logits of a chunk and one of the best so far
struct LpSel {
    uint64_t heads[256];
    uint64_t cand[LP_TOP * LP_MAX_M];
    uint64_t top[LP_TOP];
    uint64_t thr;
    int cnt;
};

// the LP_TOP largest of the block's 256 x M keys -> sh.top[0 .. LP_TOP - 1], descending, 0 where there are fewer; all 256 threads, ends with a barrier
template <int M>
__device__ __forceinline__ void lp_top20(const uint64_t (&k)[M], LpSel& sh) {
    static_assert(M <= LP_MAX_M, "the candidate list holds LP_TOP threads' keys");
    const int tid = threadIdx.x;
    uint64_t head = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) head = k[j] > head ? k[j] : head;
    __syncthreads();                                                // whoever read sh before is done
    sh.heads[tid] = head;
    if (tid < LP_TOP) sh.top[tid] = 0;
    if (tid == 0) { sh.thr = 0; sh.cnt = 0; }
    __syncthreads();
    int above = 0;
    for (int j = 0; j < 256; ++j) above += sh.heads[j] > head ? 1 : 0;
    if (above == LP_TOP - 1) sh.thr = head;                         // (fewer than 20 heads: nobody, or threads without a key writing the 0 it holds)
    __syncthreads();
    const uint64_t T = sh.thr;
    if (head != 0 && head >= T) {                                   // at most LP_TOP threads: heads are distinct
#pragma unroll
        for (int j = 0; j < M; ++j)
            if (k[j] != 0 && k[j] >= T) {
                const int at = atomicAdd(&sh.cnt, 1);
                if (at < LP_TOP * LP_MAX_M) sh.cand[at] = k[j];     // (always: see above; a list that cannot overflow whatever the keys)
            }
    }
    __syncthreads();
    const int C = sh.cnt < LP_TOP * LP_MAX_M ? sh.cnt : LP_TOP * LP_MAX_M;
    for (int i = tid; i < C; i += 256) {
        const uint64_t me = sh.cand[i];
        int rank = 0;
        for (int j = 0; j < C; ++j) rank += sh.cand[j] > me ? 1 : 0;
        if (rank < LP_TOP) sh.top[rank] = me;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void lp_slice_kernel(const float* __restrict__ logits, int64_t ld, int V, int per, uint64_t* __restrict__ wkeys,
                                                       float* __restrict__ wms) {
    __shared__ LpSel sel;
    __shared__ float fred[4];
    const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int64_t lo = (int64_t)sl * per;                           // < V: the grid has lp_slices(V) columns
    const int64_t hi = lo + per < (int64_t)V ? lo + per : (int64_t)V;
    const float* lr = logits + (int64_t)row * ld;
    if (tid < LP_TOP) sel.top[tid] = 0;                             // below every real key
    float m_run = -INFINITY, s_run = 0.f;
    for (int64_t c = lo; c < hi; c += LP_CHUNK) {
        __syncthreads();                                            // sel.top[] of the chunk before (or its zeros), fred[] free again
        float x[16];
        uint64_t k[17];
        const bool vec = ((uintptr_t)(lr + c) & 15) == 0;           // block-uniform
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = c + 1024 * q + 4 * tid;
            if (i + 4 <= hi && vec) {
                const f32x4 v = *(const f32x4*)(lr + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * q + j] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * q + j] = i + j < hi ? lr[i + j] : -INFINITY;
            }
            // (x + 0: -0.0 orders as +0.0, a comparison of floats sees them equal and the lower index wins)
#pragma unroll
            for (int j = 0; j < 4; ++j) k[4 * q + j] = i + j < hi ? smp_key(x[4 * q + j] + 0.f, (int)(i + j)) : 0;
        }
        k[16] = tid < LP_TOP ? sel.top[tid] : 0;                    // the best of the chunks before compete as a 17th element
        lp_top20<17>(k, sel);
        // the largest key holds the largest value seen so far in this slice (the chunk is not empty: it is a real key)
        const float m_new = smp_val(sel.top[0]);
        // ---- sum exp(x - m_new) of the chunk, and the running pair rescaled to m_new ----
        float ts = 0.f;
        if (m_new > -INFINITY) {
#pragma unroll
            for (int j = 0; j < 16; ++j) ts += expf(x[j] - m_new);  // an element beyond the row is -inf: exp = 0
        }
        ts = wave_sum(ts);
        if ((tid & 63) == 0) fred[wave] = ts;
        __syncthreads();
        const float total = ((fred[0] + fred[1]) + fred[2]) + fred[3];
        s_run = m_new > -INFINITY ? s_run * expf(m_run - m_new) + total : 0.f;      // (m_run = -inf: s_run is 0 and exp gives 0)
        m_run = m_new;
    }
    __syncthreads();
    const int64_t o = (int64_t)row * LP_MAX_SLICES + sl;
    if (tid < LP_TOP) wkeys[o * LP_TOP + tid] = sel.top[tid];
    if (tid == 0) { wms[2 * o] = m_run; wms[2 * o + 1] = s_run; }
}

__global__ __launch_bounds__(256) void lp_final_kernel(const float* __restrict__ logits, int64_t ld, int V, int n_slices, const uint64_t* __restrict__ wkeys,
                                                       const float* __restrict__ wms, const int64_t* __restrict__ token, int top_n,
                                                       const int32_t* __restrict__ rec, int rec_bias, float* __restrict__ token_lp, float* __restrict__ top_lp,
                                                       int32_t* __restrict__ top_id, int max_rec, int one_seq) {
    __shared__ LpSel sel;
    __shared__ float ms[2 * LP_MAX_SLICES];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int64_t r = (int64_t)(rec != nullptr ? rec[row] : 0) + rec_bias;
    if (r < 0 || r >= (int64_t)max_rec) return;                     // block-uniform: no record, nothing written
    // everything the block reads from memory is asked for up front: the candidates, the slices' (max, sum) pairs and the chosen token's logit
    const uint64_t* kr = wkeys + (int64_t)row * LP_ROW_KEYS;
    uint64_t k[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) k[q] = tid + 256 * q < n_slices * LP_TOP ? kr[tid + 256 * q] : 0;
    if (tid < 2 * n_slices) ms[tid] = wms[(int64_t)row * LP_MAX_SLICES * 2 + tid];
    float xt = __uint_as_float(0x7fc00000u);                       // a token outside the vocabulary: NaN
    if (tid == 0) {
        const int64_t t = token[row];
        if (t >= 0 && t < (int64_t)V) xt = logits[(int64_t)row * ld + t];
    }
    lp_top20<4>(k, sel);                                            // (its barriers also publish ms[])
    if (tid >= LP_TOP) return;
    float M = -INFINITY;
    for (int s = 0; s < n_slices; ++s) M = fmaxf(M, ms[2 * s]);
    float L = 0.f;
    for (int s = 0; s < n_slices; ++s) { const float m = ms[2 * s]; if (m > -INFINITY) L += ms[2 * s + 1] * expf(m - M); }
    const float lse = M + logf(L);
    const int64_t o = (one_seq ? (int64_t)0 : (int64_t)row * max_rec) + r;      // one_seq: every row is a step of ONE sequence and writes output row 0
    if (tid == 0) token_lp[o] = xt - lse;
    if (top_lp != nullptr) {
        const uint64_t best = sel.top[tid];
        const bool real = best != 0 && tid < top_n;
        top_id[o * LP_TOP + tid] = real ? smp_idx(best) : -1;
        top_lp[o * LP_TOP + tid] = real ? smp_val(best) - lse : -INFINITY;
    }
}

int launch_logprobs(const float* logits, int64_t ld, int n, int vocab, const int64_t* token, int top_n, const int32_t* rec, int rec_bias, float* token_lp,
                    float* top_lp, int32_t* top_id, int max_rec, void* workspace, hipStream_t s, bool one_seq) {
    static_assert(LP_TOP == 20 && LP_MAX_SLICES * LP_TOP <= 4 * 256, "stage 2 holds the candidates of a row as four keys per thread");
    VILA_REQUIRE(logits != nullptr && token != nullptr && token_lp != nullptr && workspace != nullptr, "logprobs: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 65535 && vocab >= 1, "logprobs: 1..65535 rows of a non-empty vocabulary (got %d x %d)", n, vocab);
    VILA_REQUIRE(top_n >= 0 && top_n <= LP_TOP, "logprobs: top_n must be in 0..%d (got %d)", LP_TOP, top_n);
    VILA_REQUIRE(ld >= vocab, "logprobs: the row stride %lld is below the vocabulary %d", (long long)ld, vocab);
    VILA_REQUIRE((top_lp == nullptr) == (top_id == nullptr), "logprobs: the alternatives need both top_logprob and top_id, or neither");
    VILA_REQUIRE(top_n == 0 || top_lp != nullptr, "logprobs: top_n = %d needs the top_logprob / top_id buffers", top_n);
    VILA_REQUIRE(max_rec >= 1, "logprobs: max_rec must be >= 1 (got %d)", max_rec);
    const int per = logprob_slice_width(vocab), ns = lp_slices(vocab);
    uint64_t* wkeys = (uint64_t*)workspace;
    float* wms = (float*)(wkeys + (size_t)n * LP_ROW_KEYS);
    hipLaunchKernelGGL(lp_slice_kernel, dim3(ns, n), dim3(256), 0, s, logits, ld, vocab, per, wkeys, wms);
    VILA_LAUNCH_CHECK();
    hipLaunchKernelGGL(lp_final_kernel, dim3(n), dim3(256), 0, s, logits, ld, vocab, ns, (const uint64_t*)wkeys, (const float*)wms, token, top_n, rec, rec_bias,
                       token_lp, top_lp, top_id, max_rec, one_seq ? 1 : 0);
    VILA_LAUNCH_CHECK();
    return 0;
}

// The records of a verify step (decode_batch.hip bverify_step), behind its accept: with m = *n_accept and old = *n_out - (m + 1), row i <= m emitted
// out_ids[old + i], which goes into record old + i of the ONE sequence's arrays; a row behind m (a rejected draft, padding) gets record -1 and writes
// nothing, and so does an id the guarded out_ids never held.  One wave writes tok_rows[i] / rec_rows[i] for launch_logprobs(one_seq).
__global__ __launch_bounds__(64) void lp_verify_index_kernel(const int64_t* __restrict__ out_ids, const int32_t* __restrict__ n_out, const int32_t* __restrict__ n_accept,
                                                             int n, int max_out, int64_t* __restrict__ tok_rows, int32_t* __restrict__ rec_rows) {
    const int i = threadIdx.x;
    if (i >= n) return;
    int m = *n_accept;
    m = m < 0 ? 0 : (m > n - 1 ? n - 1 : m);
    const int64_t k = (int64_t)*n_out - (m + 1) + i;
    const bool live = i <= m && k >= 0 && k < (int64_t)max_out;
    tok_rows[i] = live ? out_ids[k] : (int64_t)-1;
    rec_rows[i] = live ? (int32_t)k : -1;
}
int launch_logprobs_verify_index(const int64_t* out_ids, const int32_t* n_out, const int32_t* n_accept, int n, int max_out, int64_t* tok_rows, int32_t* rec_rows,
                                 hipStream_t s) {
    VILA_REQUIRE(out_ids != nullptr && n_out != nullptr && n_accept != nullptr && tok_rows != nullptr && rec_rows != nullptr && n >= 1 && n <= 64 && max_out >= 1,
                 "logprobs (verify index): NULL argument, or not 1..64 rows");
    hipLaunchKernelGGL(lp_verify_index_kernel, dim3(1), dim3(64), 0, s, out_ids, n_out, n_accept, n, max_out, tok_rows, rec_rows);
    VILA_LAUNCH_CHECK();
    return 0;
}

// Stochastic next-token choice for generate(do_sample=True) — the reference's server default (server.py:101-102,185-187: temperature 0.2,
// top_p 0.9, do_sample = temperature > 0; HF GenerationConfig's default top_k = 50 stays in force).  HF order of operations
// (GenerationMixin._get_logits_processor + sample): logits / temperature -> TopK (keep the k largest) -> TopP (ascending cumulative
// softmax, drop while cum <= 1 - top_p, keep at least one) -> softmax over what is left -> multinomial.
//
// Everything stays on the device so that a sampled decode step replays from a hipGraph like the greedy one:
//   stage 1  256 blocks: each sorts its slice of the vocabulary (bitonic, LDS) and emits its 64 best (value, index) pairs
//   stage 2  16 blocks : 1024 candidates each -> 64 best;   stage 3  1 block: 1024 -> the global top 64 (descending), then ONE wave applies
//            temperature / top-k / top-p and draws from the renormalised set with a counter-based uniform: splitmix64(seed, *counter) —
//            `counter` is the device-resident position of the token, so every replay of the captured step draws a fresh number.
// That path serves top_k in 1..64 (64 candidates survive the selection).  Any other top_k — 0 = no top-k filter, as HF treats it, or k > 64 up to
// the vocabulary — goes through smp_large_kernel below: ONE 1024-thread block, radix selection over the 64-bit (value, index) keys for the k-th
// largest, a mass-weighted radix descent for the nucleus threshold, a draw by prefix sums in index order.  The draw cannot match
// torch.multinomial's generator bit for bit — parity for this op is distributional (tests/test_gpu_sampling.py).
// The batched sampler at the end of the file makes the same choice for up to 16 rows at once (rows on blockIdx.y, per-row parameters in device
// arrays, greedy rows beside sampled ones): the pick of a batched decode step whose ONE captured graph serves any mix of requests.  It serves
// top_k in 1..64 and clamps anything else; with any_k (opt-in) rows with top_k = 0 or > 64 are drawn by smp_batch_large_kernel, one block per row.
#include "kernels.h"

#define SMP_CAND 64
#define SMP_S1_BLOCKS 256
#define SMP_S2_BLOCKS 16

// smp_key / smp_val / smp_idx live in kernels.h: logprob.hip orders its alternatives with the same keys

// descending bitonic sort of 1024 keys in LDS by 256 threads
__device__ void smp_sort1024(uint64_t* keys) {
    for (int size = 2; size <= 1024; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < 512; t += 256) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
            }
        }
    __syncthreads();
}

// a greedy row needs the largest key only: keys[0] = max of the 1024, keys[1..63] = 0 (256 threads)
__device__ void smp_max1024(uint64_t* keys) {
    __shared__ uint64_t wm[4];
    __syncthreads();
    uint64_t m = 0;
    for (int i = threadIdx.x; i < 1024; i += 256) { const uint64_t k = keys[i]; m = k > m ? k : m; }
    for (int o = 32; o > 0; o >>= 1) { const uint64_t t = __shfl_xor((unsigned long long)m, o, 64); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x < SMP_CAND) {
        uint64_t b = 0;
        for (int w = 0; w < 4; ++w) b = wm[w] > b ? wm[w] : b;
        keys[threadIdx.x] = threadIdx.x == 0 ? b : 0;
    }
    __syncthreads();
}

// stage 1 / 2: candidates in, SMP_CAND best per block out.  in_keys == nullptr: read raw logits [n] (index = position);
// otherwise read (key) candidates produced by the previous stage.  Rows of a batch lie on blockIdx.y (in_stride / out_stride elements apart);
// row_temperature (nullable, device): row `row` reads entry row * param_stride (1: an entry per row; 0: every row reads entry 0 of a one-entry
// array); a row whose temperature is not positive is a greedy row and keeps its largest key only.  row_top_k (nullable, device, read like
// row_temperature; the any-top_k sampler only): a LARGE row (smp_row_large) is drawn by smp_batch_large_kernel from the logits themselves, so its
// candidates are never read and it takes the greedy row's cheap route too.  nullptr: no row is large here.
__device__ __forceinline__ bool smp_row_large(float temperature, int top_k) {       // launch_sample's own route to smp_large_kernel
    return temperature > 0.f && (top_k == 0 || top_k > SMP_CAND);
}
__global__ __launch_bounds__(256) void smp_select_kernel(const float* __restrict__ logits, const uint64_t* __restrict__ in_keys, int n, int per_block,
                                                         uint64_t* __restrict__ out_keys, int64_t in_stride, int64_t out_stride,
                                                         const float* __restrict__ row_temperature, int param_stride,
                                                         const int32_t* __restrict__ row_top_k) {
    __shared__ uint64_t keys[1024];
    const int row = blockIdx.y;
    const float* lr = logits != nullptr ? logits + row * in_stride : nullptr;
    const uint64_t* kr = in_keys != nullptr ? in_keys + row * in_stride : nullptr;
    const int base = blockIdx.x * per_block;
    for (int i = threadIdx.x; i < 1024; i += 256) {
        const int g = base + i;
        uint64_t k = 0;                                             // below every real key
        if (i < per_block && g < n) k = (kr != nullptr) ? kr[g] : smp_key(lr[g], g);
        keys[i] = k;
    }
    bool cheap = false;                                             // block-uniform
    if (row_temperature != nullptr) {
        const float t = row_temperature[row * param_stride];
        cheap = !(t > 0.f) || (row_top_k != nullptr && smp_row_large(t, row_top_k[row * param_stride]));
    }
    if (cheap) smp_max1024(keys);
    else smp_sort1024(keys);
    if (threadIdx.x < SMP_CAND) out_keys[row * out_stride + blockIdx.x * SMP_CAND + threadIdx.x] = keys[threadIdx.x];
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The draw, by ONE wave over the sorted candidates keys[0..63] (descending): temperature / top-k / top-p, then a counter-based uniform.  Shared by
// the solo and the batched final stage, so that both make the same choice bit for bit.  Returns the token in every lane.
__device__ __forceinline__ int smp_draw_wave(const uint64_t* keys, int lane, float inv_temperature, int top_k, float top_p, uint64_t seed, uint32_t counter,
                                             float* __restrict__ prob_out) {
    const uint64_t k = keys[lane];
    // TopK: the k most likely survive.  A -inf candidate (a masked token: constrain.hip; fewer finite entries than top_k) is no candidate: its mass is
    // zero, but the lane sums of `cum` below are rounded per lane, so it could still win the draw.  Rows without -inf keep their bits.
    const bool real = k != 0 && lane < top_k && smp_val(k) != -INFINITY;
    const float z = smp_val(k) * inv_temperature, zmax = smp_val(keys[0]) * inv_temperature;
    const float e = real ? __expf(z - zmax) : 0.f;
    const float total = wave_sum(e);
    const float p = e / total;                                      // softmax over the top-k set (descending order by construction)
    // exclusive prefix sum over the wave (descending probabilities)
    float incl = p;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const float before = incl - p;                                  // probability mass of strictly more likely tokens
    const bool keep = real && (lane == 0 || before < top_p);        // TopP (HF keeps the token that crosses the threshold; at least one)
    const float pk = keep ? p : 0.f;
    const float kept_total = wave_sum(pk);
    float cum = pk;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(cum, o, 64);
        if (lane >= o) cum += t;
    }
    const uint64_t r = splitmix64(seed ^ splitmix64((uint64_t)counter));
    const float u = (float)(r >> 40) * (1.0f / 16777216.0f) * kept_total;      // uniform in [0, kept_total)
    const unsigned long long hit = __ballot(keep && cum > u);
    const int pick = hit ? __ffsll((long long)hit) - 1 : 0;
    if (prob_out != nullptr) prob_out[lane] = pk / kept_total;     // optional: the distribution that was sampled (tests)
    if (prob_out != nullptr) ((int*)(prob_out + 64))[lane] = real ? smp_idx(k) : -1;
    return __shfl(smp_idx(k), pick, 64);
}

// stage 3: global top-64, then temperature / top-k / top-p / draw by wave 0
__global__ __launch_bounds__(256) void smp_final_kernel(const uint64_t* __restrict__ in_keys, int n_in, float inv_temperature, int top_k, float top_p,
                                                        uint64_t seed_imm, const uint64_t* __restrict__ seed_dev, const int32_t* __restrict__ counter, int64_t* __restrict__ out, float* __restrict__ prob_out) {
    __shared__ uint64_t keys[1024];
    for (int i = threadIdx.x; i < 1024; i += 256) keys[i] = i < n_in ? in_keys[i] : 0;
    smp_sort1024(keys);
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const uint64_t seed = seed_dev != nullptr ? *seed_dev : seed_imm;
    const int tok = smp_draw_wave(keys, lane, inv_temperature, top_k, top_p, seed, (uint32_t)(counter != nullptr ? *counter : 0), prob_out);
    if (lane == 0) *out = (int64_t)tok;
}

// stage 3 of the batched sampler: one block per row.  Every per-row parameter is read from device arrays, so ONE captured launch serves any mix
// of rows: temperature <= 0 = greedy row (the largest key: highest value, ties to the lower index).  top_k / top_p are clamped to 1..64 / (0, 1]
// (the host validates; a bad device value must not index out of range).  adv_pos != nullptr: the state advance of the batched decode step
// (bdec_pick2_kernel's), with `counter` read BEFORE the position moves (counter and adv_pos are the same array there: no __restrict__).
// param_stride: 1 = row `row` reads entry `row` of the four parameter arrays (the batched step: one request per row); 0 = every row reads entry 0
// (the sampled verify step: n rows of ONE request, arrays of one entry).  counter / out / prob_out / adv_* stay per row either way.
// large_tok (nullable; the any-top_k sampler only): a LARGE row (smp_row_large) was drawn by smp_batch_large_kernel, which ran BEFORE this launch;
// the row skips sort and draw, takes large_tok[row], and is written and advanced here like every other row (prob_out: zeros and -1 ids, the row's
// distribution is the dense one of that kernel).  nullptr: no row is large, and top_k is clamped as ever.
__global__ __launch_bounds__(256) void smp_batch_final_kernel(const uint64_t* __restrict__ in_keys, int n_in, int64_t in_stride, const float* __restrict__ temperature,
                                                              const int32_t* __restrict__ top_k, const float* __restrict__ top_p, const uint64_t* __restrict__ seed,
                                                              const int32_t* counter, int64_t* __restrict__ out, float* __restrict__ prob_out,
                                                              int32_t* adv_pos, int64_t* __restrict__ adv_out_ids, int32_t* __restrict__ adv_n_out, int max_out,
                                                              int param_stride, const int64_t* __restrict__ large_tok) {
    __shared__ uint64_t keys[1024];
    const int row = blockIdx.x, prow = row * param_stride;
    const float t = temperature[prow];
    const bool sampled = t > 0.f;                                   // block-uniform
    const bool large = large_tok != nullptr && smp_row_large(t, top_k[prow]);       // block-uniform
    if (!large) {
        for (int i = threadIdx.x; i < 1024; i += 256) keys[i] = i < n_in ? in_keys[row * in_stride + i] : 0;
        if (sampled) smp_sort1024(keys); else smp_max1024(keys);
    }
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const uint32_t ctr = counter != nullptr ? (uint32_t)counter[row] : 0u;
    float* pr = prob_out != nullptr ? prob_out + (int64_t)row * 2 * SMP_CAND : nullptr;
    int tok;
    if (large) {
        tok = (int)large_tok[row];
        if (pr != nullptr) { pr[lane] = 0.f; ((int*)(pr + 64))[lane] = -1; }
    } else if (sampled) {
        int k = top_k[prow];
        k = k < 1 ? 1 : (k > SMP_CAND ? SMP_CAND : k);
        const float p = fminf(fmaxf(top_p[prow], 1.17549435e-38f), 1.0f);
        tok = smp_draw_wave(keys, lane, 1.0f / t, k, p, seed[prow], ctr, pr);
    } else {
        tok = smp_idx(keys[0]);
        if (pr != nullptr) { pr[lane] = lane == 0 ? 1.f : 0.f; ((int*)(pr + 64))[lane] = lane == 0 ? tok : -1; }
    }
    if (lane == 0) {
        out[row] = (int64_t)tok;
        if (adv_pos != nullptr) {
            const int n = adv_n_out[row];
            if (n < max_out) adv_out_ids[(int64_t)row * max_out + n] = (int64_t)tok;
            adv_n_out[row] = n + 1;
            adv_pos[row] = (int32_t)ctr + 1;
        }
    }
}

// ---- any top_k (round 4): exact selection without a candidate cut ----------------------------------------------------------------------------
// Keys are a strict total order (value, then LOWER index first), so "the k most likely" and "the tokens whose more-likely mass is below top_p"
// are both `key >= threshold` sets:
//   T_k : 8 radix passes (one byte of the 64-bit key per pass, integer histograms) find the k-th largest key
//   T_p : 8 passes with MASS histograms (sum of exp((v - vmax) / T) per bin, accumulated as 2^-40 fixed-point integers so the sums do not depend on
//         lane arrival order; one histogram row per wave, rows added in a fixed order) descend to
//         the smallest key whose strictly-more-likely mass is still below top_p x total  (HF TopPLogitsWarper: drop while ascending cumulative
//         mass <= 1 - top_p; the top token always survives)
//   draw: u in [0, kept mass) located by prefix sums over the kept tokens in INDEX order (any fixed order gives the same distribution)
#define SMPL_T 1024
__device__ __forceinline__ float smpl_block_sum(float v, float* red) {      // fixed-order tree: the same bits on every run
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < SMPL_T / 64; ++i) t += red[i];
    return t;
}
// One block of SMPL_T threads draws ONE row: the body of the solo kernel and of the batched one below, so that both make the same choice bit for
// bit (the same per-thread strides, fixed-order reductions, fixed-point histograms and index-order draw whatever the launch).
__device__ __forceinline__ void smp_large_row(const float* __restrict__ logits, int n, float inv_temperature, int top_k, float top_p, uint64_t seed,
                                              uint32_t counter, int64_t* __restrict__ out, float* __restrict__ prob_out) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long histq[SMPL_T / 64][256];     // nucleus masses in 2^-40 fixed point: INTEGER atomics commute, so a bin's sum
                                                               // has the same bits whatever order the lanes of a wave arrive in
    __shared__ float red[SMPL_T / 64];
    __shared__ float scan[SMPL_T];
    __shared__ uint64_t sh_key;
    __shared__ float sh_f;
    __shared__ int sh_i;
    const int tid = threadIdx.x, wave = tid >> 6;
    // ---- the largest key (value -> softmax shift) ----
    uint64_t kmax = 0;
    for (int i = tid; i < n; i += SMPL_T) { const uint64_t k = smp_key(logits[i], i); kmax = k > kmax ? k : kmax; }
    for (int o = 32; o > 0; o >>= 1) { const uint64_t t = __shfl_xor((unsigned long long)kmax, o, 64); kmax = t > kmax ? t : kmax; }
    if ((tid & 63) == 0) ((uint64_t*)histq)[wave] = kmax;
    __syncthreads();
    if (tid == 0) { uint64_t m = 0; for (int w = 0; w < SMPL_T / 64; ++w) { const uint64_t t = ((uint64_t*)histq)[w]; m = t > m ? t : m; } sh_key = m; }
    __syncthreads();
    kmax = sh_key;
    const float zmax = smp_val(kmax) * inv_temperature;
    __syncthreads();
    // ---- T_k: the k-th largest key (0 = keep everything) ----
    uint64_t Tk = 0;
    if (top_k >= 1 && top_k < n) {
        uint64_t prefix = 0;
        uint32_t remaining = (uint32_t)top_k;
        for (int b = 7; b >= 0; --b) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const uint64_t hi_mask = b == 7 ? 0ull : (~0ull << (8 * (b + 1)));
            for (int i = tid; i < n; i += SMPL_T) {
                const uint64_t k = smp_key(logits[i], i);
                if ((k & hi_mask) == prefix) atomicAdd(&hist[(k >> (8 * b)) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t cum = 0; int d = 255;
                for (; d > 0; --d) { if (cum + hist[d] >= remaining) break; cum += hist[d]; }
                sh_i = d; sh_f = __uint_as_float(cum);
            }
            __syncthreads();
            prefix |= (uint64_t)sh_i << (8 * b);
            remaining -= __float_as_uint(sh_f);
            __syncthreads();
        }
        Tk = prefix;
    }
    // ---- mass of the top-k set ----
    float part = 0.f;
    for (int i = tid; i < n; i += SMPL_T) { const float v = logits[i]; if (smp_key(v, i) >= Tk) part += __expf(v * inv_temperature - zmax); }
    const float total_k = smpl_block_sum(part, red);
    // ---- T_p: the smallest key kept by the nucleus ----
    uint64_t T = Tk;
    if (top_p < 1.f) {
        const float thr = top_p * total_k;
        uint64_t prefix = 0;
        float above = 0.f;                                       // mass of the keys above the current prefix range
        for (int b = 7; b >= 0; --b) {
            for (int i = tid; i < (SMPL_T / 64) * 256; i += SMPL_T) (&histq[0][0])[i] = 0ull;
            __syncthreads();
            const uint64_t hi_mask = b == 7 ? 0ull : (~0ull << (8 * (b + 1)));
            for (int i = tid; i < n; i += SMPL_T) {
                const float v = logits[i];
                const uint64_t k = smp_key(v, i);
                if (k >= Tk && (k & hi_mask) == prefix)      // e <= 1 (shifted by the largest logit): e * 2^40 fits, 2^18 of them fit 64 bits
                    atomicAdd(&histq[wave][(k >> (8 * b)) & 255u], (unsigned long long)(__expf(v * inv_temperature - zmax) * 1099511627776.0f));
            }
            __syncthreads();
            if (tid < 256) { unsigned long long m = 0ull; for (int w = 0; w < SMPL_T / 64; ++w) m += histq[w][tid]; scan[tid] = (float)m * (1.0f / 1099511627776.0f); }
            __syncthreads();
            if (tid == 0) {
                // bins from the top: G(d) = above + mass of bins > d; descend into the LOWEST bin whose G is still below the threshold
                float g = above; int d = 255, best = -1; float gbest = above;
                for (; d >= 0; --d) {
                    if (g < thr) { if (scan[d] > 0.f || best < 0) { best = d; gbest = g; } } else break;
                    g += scan[d];
                }
                if (best < 0) { best = 255; gbest = above; }
                // (only non-empty bins can hold the threshold key; the top bin of the first pass holds the largest key, which is always kept)
                sh_i = best; sh_f = gbest;
            }
            __syncthreads();
            prefix |= (uint64_t)sh_i << (8 * b);
            above = sh_f;
            __syncthreads();
        }
        T = prefix > Tk ? prefix : Tk;
    }
    // ---- draw in index order ----
    const int chunk = (n + SMPL_T - 1) / SMPL_T, i0 = tid * chunk, i1 = (i0 + chunk < n) ? i0 + chunk : n;
    float mine = 0.f;
    for (int i = i0; i < i1; ++i) { const float v = logits[i]; if (smp_key(v, i) >= T) mine += __expf(v * inv_temperature - zmax); }
    scan[tid] = mine;
    __syncthreads();
    if (tid == 0) {                                              // 1024 partials: a serial scan by one thread keeps the order fixed
        float acc = 0.f;
        for (int t = 0; t < SMPL_T; ++t) { const float m = scan[t]; scan[t] = acc; acc += m; }
        sh_f = acc;
        sh_i = -1;
    }
    __syncthreads();
    const float kept_total = sh_f;
    const uint64_t r = splitmix64(seed ^ splitmix64((uint64_t)counter));
    const float u = (float)(r >> 40) * (1.0f / 16777216.0f) * kept_total;
    const float base = scan[tid];
    if (mine > 0.f && u >= base && (u < base + mine || tid == SMPL_T - 1)) {
        float acc = base; int pick = -1, last = -1;
        for (int i = i0; i < i1; ++i) {
            const float v = logits[i];
            if (smp_key(v, i) >= T) { if (v != -INFINITY) last = i; acc += __expf(v * inv_temperature - zmax); if (pick < 0 && u < acc) pick = i; }   // (a -inf entry, a masked token, is never the fallback)
        }
        atomicMax(&sh_i, pick >= 0 ? pick : last);               // (at most one chunk contains u; rounding at a chunk edge: the later one wins)
    }
    __syncthreads();
    if (tid == 0) *out = (int64_t)(sh_i >= 0 ? sh_i : smp_idx(kmax));      // u beyond the last partial by rounding: the most likely token
    if (prob_out != nullptr)
        for (int i = tid; i < n; i += SMPL_T) { const float v = logits[i]; prob_out[i] = smp_key(v, i) >= T ? __expf(v * inv_temperature - zmax) / kept_total : 0.f; }
}
__global__ __launch_bounds__(SMPL_T) void smp_large_kernel(const float* __restrict__ logits, int n, float inv_temperature, int top_k, float top_p,
                                                           uint64_t seed_imm, const uint64_t* __restrict__ seed_dev, const int32_t* __restrict__ counter,
                                                           int64_t* __restrict__ out, float* __restrict__ prob_out) {
    smp_large_row(logits, n, inv_temperature, top_k, top_p, seed_dev != nullptr ? *seed_dev : seed_imm, (uint32_t)(counter != nullptr ? *counter : 0), out,
                  prob_out);
}
// The batched form: one block per row of logits [rows][ld_logits], the row's parameters read from the device arrays as smp_batch_final_kernel reads
// them (param_stride 1 or 0), the counter from counter[row].  Only a LARGE row (smp_row_large: launch_sample's route to the kernel above, so the
// bits are the solo path's) is drawn; every other block returns at once (the branch is block-uniform).  The token goes to large_tok[row], which
// smp_batch_final_kernel reads: the row's `out` and its state advance stay in that kernel, which therefore runs AFTER this one — counter and the
// advanced position are the same array in the decode step, and it must be read here before it moves.  top_p is clamped to (0, 1] as the final
// kernel clamps it (an identity on what the host admits).  dense_out (nullable): the row's distribution [vocab] at dense_out + row * ld_dense.
__global__ __launch_bounds__(SMPL_T) void smp_batch_large_kernel(const float* __restrict__ logits, int64_t ld_logits, int vocab, const float* __restrict__ temperature,
                                                                 const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                                 const uint64_t* __restrict__ seed, const int32_t* __restrict__ counter,
                                                                 int64_t* __restrict__ large_tok, float* __restrict__ dense_out, int64_t ld_dense, int param_stride) {
    const int row = blockIdx.x, prow = row * param_stride;
    const float t = temperature[prow];
    const int k = top_k[prow];
    if (!smp_row_large(t, k)) return;                              // block-uniform
    const float p = fminf(fmaxf(top_p[prow], 1.17549435e-38f), 1.0f);
    smp_large_row(logits + (int64_t)row * ld_logits, vocab, 1.0f / t, k, p, seed[prow], counter != nullptr ? (uint32_t)counter[row] : 0u, large_tok + row,
                  dense_out != nullptr ? dense_out + (int64_t)row * ld_dense : nullptr);
}

size_t sample_workspace_bytes() { return (size_t)(SMP_S1_BLOCKS + SMP_S2_BLOCKS) * SMP_CAND * sizeof(uint64_t) + 256; }

int launch_sample(const float* logits, int n, float temperature, int top_k, float top_p, uint64_t seed, const uint64_t* seed_dev, const int32_t* counter, int64_t* out,
                  void* workspace, float* prob_out, hipStream_t s) {
    VILA_REQUIRE(n > 0 && temperature > 0.f, "sample: temperature must be positive (got %g); use greedy search for temperature 0", (double)temperature);
    VILA_REQUIRE(top_k >= 0, "sample: top_k must be >= 0 (got %d; 0 = no top-k filter)", top_k);
    VILA_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample: top_p must be in (0, 1] (got %g)", (double)top_p);
    if (top_k == 0 || top_k > SMP_CAND) {                       // any k: exact radix selection in one block (prob_out: dense [n])
        hipLaunchKernelGGL(smp_large_kernel, dim3(1), dim3(SMPL_T), 0, s, logits, n, 1.0f / temperature, top_k, top_p, seed, seed_dev, counter, out, prob_out);
        VILA_LAUNCH_CHECK();
        return 0;
    }
    const int per1 = cdiv(n, SMP_S1_BLOCKS);
    VILA_REQUIRE(per1 <= 1024, "sample: vocabulary of %d exceeds %d x 1024 entries", n, SMP_S1_BLOCKS);
    uint64_t* c1 = (uint64_t*)workspace;
    uint64_t* c2 = c1 + SMP_S1_BLOCKS * SMP_CAND;
    hipLaunchKernelGGL(smp_select_kernel, dim3(SMP_S1_BLOCKS), dim3(256), 0, s, logits, (const uint64_t*)nullptr, n, per1, c1, (int64_t)0, (int64_t)0, (const float*)nullptr, 0, (const int32_t*)nullptr);
    VILA_LAUNCH_CHECK();
    hipLaunchKernelGGL(smp_select_kernel, dim3(SMP_S2_BLOCKS), dim3(256), 0, s, (const float*)nullptr, (const uint64_t*)c1, SMP_S1_BLOCKS * SMP_CAND, 1024, c2, (int64_t)0, (int64_t)0, (const float*)nullptr, 0, (const int32_t*)nullptr);
    VILA_LAUNCH_CHECK();
    hipLaunchKernelGGL(smp_final_kernel, dim3(1), dim3(256), 0, s, (const uint64_t*)c2, SMP_S2_BLOCKS * SMP_CAND, 1.0f / temperature, top_k, top_p, seed, seed_dev, counter, out, prob_out);
    VILA_LAUNCH_CHECK();
    return 0;
}

// ---- the batched sampler: one choice per row of logits [n][vocab] in three launches whatever n ------------------------------------------------
// Rows lie on blockIdx.y.  Stage 1 cuts a row into cdiv(vocab, 1024) slices of (almost) 1024 logits — full sorts, where the solo path's fixed
// 256 slices sort 594 logits and 430 pads each — stage 2 sorts 1024 candidates per block, stage 3 is one block per row.  The top-64 set under the
// strict key order does not depend on the cut, and stage 3 draws with the solo sampler's own arithmetic (smp_draw_wave).
// sp_stride: 1 = sp's arrays hold n entries, one per row; 0 = they hold ONE entry that every row reads (n rows of one request).
// any_k (opt-in; false = the three launches above, kernel for kernel, every pointer this option added NULL): a fourth launch, smp_batch_large_kernel, draws the
// rows with top_k = 0 or > 64 by the solo sampler's exact path, and the final kernel takes their tokens instead of clamping top_k to 1..64.
static inline int smpb_s1(int vocab) { return cdiv(vocab, 1024); }
static inline int smpb_s2(int vocab) { return cdiv(smpb_s1(vocab) * SMP_CAND, 1024); }
size_t sample_batch_workspace_bytes(int n) { return (size_t)(n > 0 ? n : 0) * (SMP_S1_BLOCKS + SMP_S2_BLOCKS) * SMP_CAND * sizeof(uint64_t) + 256; }

int launch_sample_batch(const float* logits, int64_t ld_logits, int n, int vocab, const BatchSampling& sp, int sp_stride, const int32_t* counter, int64_t* out,
                        void* workspace, float* dist_out, int32_t* adv_pos, int64_t* adv_out_ids, int32_t* adv_n_out, int max_out, hipStream_t s, bool any_k,
                        float* dense_out, int64_t ld_dense) {
    VILA_REQUIRE(n >= 1 && n <= 16, "sample_batch: 1..16 rows (got %d)", n);
    VILA_REQUIRE(vocab > 0 && ld_logits >= vocab, "sample_batch: row stride %lld is below the vocabulary %d", (long long)ld_logits, vocab);
    VILA_REQUIRE(smpb_s1(vocab) <= SMP_S1_BLOCKS, "sample_batch: vocabulary of %d exceeds %d x 1024 entries", vocab, SMP_S1_BLOCKS);
    VILA_REQUIRE(sp.temperature != nullptr && sp.top_k != nullptr && sp.top_p != nullptr && sp.seed != nullptr, "sample_batch: a per-row parameter array is NULL");
    VILA_REQUIRE(sp_stride == 0 || sp_stride == 1, "sample_batch: the parameter arrays hold one entry per row (stride 1) or one in all (0), got %d", sp_stride);
    VILA_REQUIRE(adv_pos == nullptr || (adv_out_ids != nullptr && adv_n_out != nullptr && max_out >= 1), "sample_batch: the state advance needs out_ids and n_out");
    VILA_REQUIRE(dense_out == nullptr || (any_k && ld_dense >= vocab), "sample_batch: the dense distribution is the any-top_k sampler's, rows of at least the vocabulary");
    const int s1 = smpb_s1(vocab), s2 = smpb_s2(vocab), per1 = cdiv(vocab, s1);
    uint64_t* c1 = (uint64_t*)workspace;
    uint64_t* c2 = c1 + (size_t)n * SMP_S1_BLOCKS * SMP_CAND;
    // any_k: the large rows' tokens, 16 int64 in the 256 trailing bytes of sample_batch_workspace_bytes(n) — c1 ends where c2 begins, c2's n rows of
    // at most SMP_S2_BLOCKS * SMP_CAND keys end at n * (SMP_S1_BLOCKS + SMP_S2_BLOCKS) * SMP_CAND keys, and nothing else lies behind them
    static_assert(16 * sizeof(int64_t) <= 256, "the large rows' tokens fit the workspace's trailing bytes");
    int64_t* large_tok = any_k ? (int64_t*)(c1 + (size_t)n * (SMP_S1_BLOCKS + SMP_S2_BLOCKS) * SMP_CAND) : nullptr;
    const int32_t* sel_k = any_k ? sp.top_k : nullptr;
    hipLaunchKernelGGL(smp_select_kernel, dim3(s1, n), dim3(256), 0, s, logits, (const uint64_t*)nullptr, vocab, per1, c1, ld_logits, (int64_t)s1 * SMP_CAND, sp.temperature, sp_stride,
                       sel_k);
    VILA_LAUNCH_CHECK();
    hipLaunchKernelGGL(smp_select_kernel, dim3(s2, n), dim3(256), 0, s, (const float*)nullptr, (const uint64_t*)c1, s1 * SMP_CAND, 1024, c2, (int64_t)s1 * SMP_CAND,
                       (int64_t)s2 * SMP_CAND, sp.temperature, sp_stride, sel_k);
    VILA_LAUNCH_CHECK();
    if (any_k) {                                                    // before the final kernel: it reads `counter`, which that kernel advances
        hipLaunchKernelGGL(smp_batch_large_kernel, dim3(n), dim3(SMPL_T), 0, s, logits, ld_logits, vocab, sp.temperature, sp.top_k, sp.top_p, sp.seed, counter, large_tok,
                           dense_out, ld_dense, sp_stride);
        VILA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(smp_batch_final_kernel, dim3(n), dim3(256), 0, s, (const uint64_t*)c2, s2 * SMP_CAND, (int64_t)s2 * SMP_CAND, sp.temperature, sp.top_k, sp.top_p, sp.seed,
                       counter, out, dist_out, adv_pos, adv_out_ids, adv_n_out, max_out, sp_stride, (const int64_t*)large_tok);
    VILA_LAUNCH_CHECK();
    return 0;
}

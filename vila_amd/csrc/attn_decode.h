// Decode attention: the pieces that more than one translation unit uses (attn_decode.hip, the o_proj GEMVs of gemv.hip and gemv_w4.hip, api.hip).
#pragma once
#include "kernels.h"

#define DEC_KS 64                        // keys per split of attn_decode_partial
#define DEC_MAXG 8                       // max query heads per kv head of attn_decode_partial
#define DEC_SHORT_CTX BDEC_SHORT_CTX     // caches up to this many positions take the single-launch per-head kernel, longer ones the split-KV pair

// The first half of the flash-decoding combine that the o_proj GEMVs run in their prologue: the weight of every slice's partial,
//   wsm[s][h] = exp(m_s - M) / sum_s exp(m_s - M) l_s   with M = max_s m_s,
// one thread per head, published to the block by the trailing barrier.  NT = the block's thread count where the kernel knows it at compile time.
template <int NT = 0>
__device__ __forceinline__ void attn_merge_weights(const float* __restrict__ part_ml, int n_active, int nq, float* wsm /* [n_active * nq] */) {
    const int tid = threadIdx.x, nt = NT > 0 ? NT : (int)blockDim.x;
    for (int h = tid; h < nq; h += nt) {
        float M = -INFINITY;
        for (int s = 0; s < n_active; ++s) M = fmaxf(M, part_ml[((int64_t)s * nq + h) * 2]);
        float L = 0.f;
        for (int s = 0; s < n_active; ++s) {
            const float* ml = part_ml + ((int64_t)s * nq + h) * 2;
            L += __expf(ml[0] - M) * ml[1];
        }
        const float invL = 1.f / L;
        for (int s = 0; s < n_active; ++s) wsm[s * nq + h] = __expf(part_ml[((int64_t)s * nq + h) * 2] - M) * invL;
    }
    __syncthreads();
}

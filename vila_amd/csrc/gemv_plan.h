// The CU map of the batch-1 decode GEMVs (gemv.hip), worked out ONCE PER LAUNCH on the host and handed to the kernel as a few ints, so that no
// wave divides on values the host already knows.  Shared by host and device; no HIP types: tests/test_gemv_plan_cpu.py compiles this header
// alone with g++ and compares it with a transcription of CuMap (gemv_common.h), whose constructor the W4 kernels still run on the device.
//
// The map itself is CuMap's, group for group: a CU owns groups {j * ncu + cu} for j < cf; with skew (ncu a multiple of 8) the remaining `rem`
// groups go to the even CUs alone, group cf * ncu + (j - cf) * n_fast + rank(cu).  An ncu that is no multiple of 8 takes the plain interleaved
// map.  What the host adds is the division: count(cu) = cf + ceil((rem - rank) / n_fast) = cf + xq + (rank < xr) with xq = rem / n_fast and
// xr = rem % n_fast (rank < n_fast), and for the interleaved map ceil((n - cu) / ncu) = xq + (cu < xr) with xq = n / ncu, xr = n % ncu.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GEMV_PLAN_HD __host__ __device__ __forceinline__
#else
#define GEMV_PLAN_HD inline
#endif

constexpr int GEMV_PLAN_INTERLEAVED = 0x3fffffff;     // cf of the plain interleaved map (CuMap's marker)
constexpr int GEMV_PLAN_MAX_CUS = 0xffff;             // ncu and xr travel as two halves of one int

struct GemvPlan {
    int ncu_xr;      // ncu | xr << 16
    int cf;          // groups every CU takes by the interleaved map, or GEMV_PLAN_INTERLEAVED
    int xq;          // see above
    GEMV_PLAN_HD int ncu() const { return ncu_xr & 0xffff; }
    GEMV_PLAN_HD int xr() const { return (int)((unsigned)ncu_xr >> 16); }
    GEMV_PLAN_HD int n_fast() const { return ncu() >> 1; }
    GEMV_PLAN_HD static int rank(int cu) { return (cu >> 3) * 4 + ((cu & 7) >> 1); }
    GEMV_PLAN_HD int count(int cu) const {
        if (cf == GEMV_PLAN_INTERLEAVED) return xq + (cu < xr() ? 1 : 0);
        const bool fast = (cu & 1) == 0;
        return cf + (fast ? xq + (rank(cu) < xr() ? 1 : 0) : 0);
    }
    GEMV_PLAN_HD int gid(int cu, int j) const {
        if (cf == GEMV_PLAN_INTERLEAVED || j < cf) return j * ncu() + cu;
        return cf * ncu() + (j - cf) * n_fast() + rank(cu);
    }
};

// host: the plan of n_groups row groups over ncu CUs (1 <= ncu <= GEMV_PLAN_MAX_CUS), `skew` groups per CU moved from the odd XCDs to the even
inline GemvPlan gemv_plan(int n_groups, int ncu, int skew) {
    GemvPlan p;
    const bool can = (ncu & 7) == 0;
    int xr;
    if (can) {
        int cf = n_groups / ncu - skew; cf = cf < 0 ? 0 : cf;
        const int rem = n_groups - cf * ncu, n_fast = ncu >> 1;
        p.cf = cf; p.xq = rem / n_fast; xr = rem % n_fast;
    } else {
        p.cf = GEMV_PLAN_INTERLEAVED; p.xq = n_groups / ncu; xr = n_groups % ncu;
    }
    p.ncu_xr = (int)((unsigned)ncu | ((unsigned)xr << 16));
    return p;
}

// q = n / d without a division on the device, for d >= 2: q = (n * udiv_magic(d)) >> 32, exact for every n with n * d < 2^32 (the magic
// exceeds 2^32 / d by at most 1, so the product exceeds n * 2^32 / d by at most n < 2^32 / d).  The QKV kernel splits a row group into
// (head, pair) this way, the attention kernel a query head into its kv head.
inline uint32_t udiv_magic(uint32_t d) { return (uint32_t)(0x100000000ull / d) + 1u; }
GEMV_PLAN_HD uint32_t udiv_by_magic(uint32_t n, uint32_t magic) { return (uint32_t)(((uint64_t)n * magic) >> 32); }

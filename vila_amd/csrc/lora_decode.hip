// LoRA adapters served unmerged in the batched decode step: every row of the step names its own adapter.  row_adapter [n] int32 holds
// a slot of the adapter bank (vila_amd/lora_serving.py AdapterBank) or -1; a value outside 0 .. capacity - 1 counts as -1.  In front of each of a
// layer's four projections the step runs, on the projection's own input,
//     shrink   T[i][0 : Rs) = s_a (x_i . A_a^T)         a = row_adapter[i], A_a [Rs][K] the slot's stacked A (q|k|v: Rs = 3 r, gate|up: 2 r, o / down: r)
//     expand   D[i][0 : N)  = sum_j T[i][seg + j] B_a[col][j]
// and the skinny GEMM adds D to its fp32 sum (decode_batch.hip bgemm_epilogue).  T and D are fp32.
//   * shrink has the matrix-core shape of bgemm_dma_kernel: rows = sequences, 16 adapter rows as the B operand of v_mfma_f32_16x16x32_bf16.  A block is
//     one (16-row tile of A, slot) pair; its 8 waves take the 64-wide k-blocks round-robin (wave w: w, w + 8, ...), the 8 partial sums meet in LDS and
//     wave 0 adds them in wave order.  The tile is multiplied with ALL rows of x, and only the rows that name the slot are stored: an MFMA output row
//     depends on its own A-operand row alone, so row i's T is the same bits whatever n and the other rows.  No atomics.
//   * expand is one thread per output column on the VALU: B is packed [r / 8][N][8] (chunk-major), so a wave's 16-B loads are one contiguous KB; the
//     products are fmaf'ed in the order j = 0 .. r - 1.  The rows' T live in LDS.
//   * a block of a slot that no row names returns before its first read of the slot; rows without an adapter get +0.0 (from the blocks of slot 0 in
//     shrink, from every block in expand) and nothing outside [n][Rs] / [n][N] is written.
#include "../../include/vila_hip.h"
#include "kernels.h"

struct LoraShrinkArgs {
    const bf16_t* x; int64_t ldx;            // [n][K]
    const bf16_t* A; int64_t slot_stride;    // [capacity][Rs][K]; slot_stride in elements
    const float* scale;                      // [capacity]
    const int32_t* row_adapter;              // [n]
    float* T; int64_t ldt;                   // [n][Rs]
    int n, Rs, K, capacity;
};

__global__ __launch_bounds__(512) void lora_shrink_kernel(LoraShrinkArgs p) {
    __shared__ float red[8 * 64 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int slot = blockIdx.y, t0 = blockIdx.x * 16;
    // rows that name this slot / no slot, as bit masks (block-uniform): lane i < n holds row i's entry, one vector load and two ballots per wave
    // (a scalar load per row, each waited for, cost 0.8 us a row)
    const int mine = lane < p.n ? p.row_adapter[lane] : slot + 1;
    const unsigned use = (unsigned)__ballot(lane < p.n && mine == slot);
    const unsigned none = (unsigned)__ballot(lane < p.n && (mine < 0 || mine >= p.capacity));
    if (slot == 0 && wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = lg * 4 + r;
            if ((none >> m) & 1u) p.T[(int64_t)m * p.ldt + t0 + l15] = 0.f;
        }
    }
    if (use == 0) return;
    // operands straight from memory: lane (row l15, k-group lg) holds elements lg * 16 .. + 15 of the k-block, the first 8 for the first MFMA, the
    // other 8 for the second: the same deal on both sides, and a row's 128-B line is read by 4 adjacent lane groups
    const int mx = l15 < p.n ? l15 : p.n - 1;                                            // (rows beyond the batch: a copy of the last one, never stored)
    const bf16_t* xp = p.x + (int64_t)mx * p.ldx + lg * 16;
    const bf16_t* ap = p.A + (int64_t)slot * p.slot_stride + (int64_t)(t0 + l15) * p.K + lg * 16;
    const int nkb = p.K >> 6;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    // four of the wave's k-blocks per round, all sixteen loads issued before the first MFMA (a wave of down_proj walks 37 k-blocks: one round trip
    // per k-block was most of the kernel's time); the MFMAs run in k order whatever the round, so the sum does not depend on it
    int kb = wave;
    for (; kb + 24 < nkb; kb += 32) {
        u32x4 xv[8], av[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xv[2 * j] = *(const u32x4*)(xp + (kb + 8 * j) * 64); xv[2 * j + 1] = *(const u32x4*)(xp + (kb + 8 * j) * 64 + 8);
            av[2 * j] = *(const u32x4*)(ap + (kb + 8 * j) * 64); av[2 * j + 1] = *(const u32x4*)(ap + (kb + 8 * j) * 64 + 8);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xv[j]), __builtin_bit_cast(bf16x8, av[j]), acc, 0, 0, 0);
    }
    for (; kb < nkb; kb += 8) {
        const u32x4 x0 = *(const u32x4*)(xp + kb * 64), x1 = *(const u32x4*)(xp + kb * 64 + 8);
        const u32x4 a0 = *(const u32x4*)(ap + kb * 64), a1 = *(const u32x4*)(ap + kb * 64 + 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x0), __builtin_bit_cast(bf16x8, a0), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x1), __builtin_bit_cast(bf16x8, a1), acc, 0, 0, 0);
    }
    *(f32x4*)(red + (wave * 64 + lane) * 4) = acc;
    __syncthreads();
    if (wave != 0) return;
    f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const f32x4 a = *(const f32x4*)(red + (w * 64 + lane) * 4);
        sum[0] += a[0]; sum[1] += a[1]; sum[2] += a[2]; sum[3] += a[3];
    }
    const float sc = p.scale[slot];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                                        // C layout: sequence m = lg * 4 + r, adapter row t0 + l15
        const int m = lg * 4 + r;
        if ((use >> m) & 1u) p.T[(int64_t)m * p.ldt + t0 + l15] = sum[r] * sc;
    }
}

int launch_lora_shrink(const bf16_t* x, int64_t ldx, int n, const bf16_t* A, int64_t slot_stride, const float* scale, const int32_t* row_adapter, int capacity,
                       float* T, int64_t ldt, int Rs, int K, hipStream_t s) {
    VILA_REQUIRE(x != nullptr && A != nullptr && scale != nullptr && row_adapter != nullptr && T != nullptr, "lora shrink: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 16, "lora shrink: 1..16 sequences (got %d)", n);
    VILA_REQUIRE(capacity >= 1 && capacity <= LORA_MAX_SLOTS, "lora shrink: 1..%d slots (got %d)", LORA_MAX_SLOTS, capacity);
    VILA_REQUIRE(K > 0 && K % 64 == 0 && Rs > 0 && Rs % 16 == 0, "lora shrink: K (%d) must be a positive multiple of 64, the stacked rank (%d) of 16", K, Rs);
    VILA_REQUIRE(ldx >= K && ldx % 8 == 0 && ldt >= Rs && slot_stride >= (int64_t)Rs * K && slot_stride % 8 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)A % 16 == 0,
                 "lora shrink: operand alignment, or a stride shorter than what it spans");
    LoraShrinkArgs a{x, ldx, A, slot_stride, scale, row_adapter, T, ldt, n, Rs, K, capacity};
    hipLaunchKernelGGL(lora_shrink_kernel, dim3(Rs / 16, capacity), dim3(512), 0, s, a);
    VILA_LAUNCH_CHECK();
    return 0;
}

struct LoraExpandArgs {
    const float* T; int64_t ldt;             // [n][segments * r]
    const bf16_t* B; int64_t slot_stride;    // [capacity][r / 8][N][8]; slot_stride in elements
    const int32_t* row_adapter;              // [n]
    float* D; int64_t ldd;                   // [n][N]
    int n, N, c1, c2, capacity;              // columns [0, c1) read T[0 : r), [c1, c2) T[r : 2 r), [c2, N) T[2 r : 3 r)
};

template <int R>
__global__ __launch_bounds__(256) void lora_expand_kernel(LoraExpandArgs p) {
    __shared__ __attribute__((aligned(16))) float ts[16 * 3 * R];
    __shared__ int ra[16];
    __shared__ int used_slot[16], used_rows[16], n_used, no_slot;                        // the slots that rows name, in slot order, with their rows as bit masks
    const int tid = threadIdx.x;
    const int Rs = (1 + (p.c1 < p.N) + (p.c2 < p.N)) * R;
    if (tid < 64) {                                                                      // wave 0: lane i < n holds row i's entry; one ballot per slot
        int a = tid < p.n ? p.row_adapter[tid] : -1;
        a = (a < 0 || a >= p.capacity) ? -1 : a;
        if (tid < 16) ra[tid] = a;
        const unsigned none = (unsigned)__ballot(tid < p.n && a < 0);
        int k = 0;
        for (int slot = 0; slot < p.capacity; ++slot) {
            const unsigned rows = (unsigned)__ballot(a == slot);
            if (rows != 0) {
                if (tid == 0) { used_slot[k] = slot; used_rows[k] = (int)rows; }
                ++k;
            }
        }
        if (tid == 0) { n_used = k; no_slot = (int)none; }
    }
    __syncthreads();
    for (int e = tid; e < p.n * Rs; e += 256) {
        const int i = e / Rs, j = e - i * Rs;
        ts[e] = ra[i] >= 0 ? p.T[(int64_t)i * p.ldt + j] : 0.f;                          // (a row without an adapter: its T is not read)
    }
    __syncthreads();
    const int col = blockIdx.x * 256 + tid;
    if (col >= p.N) return;
    const int off = col < p.c1 ? 0 : (col < p.c2 ? R : 2 * R);
    for (unsigned m = (unsigned)no_slot; m != 0; m &= m - 1) p.D[(int64_t)(__ffs(m) - 1) * p.ldd + col] = 0.f;
    const int nu = n_used;
    for (int k = 0; k < nu; ++k) {
        const int slot = used_slot[k];
        const u32x4* bp = (const u32x4*)(p.B + (int64_t)slot * p.slot_stride) + col;
        u32x4 w[R / 8];
#pragma unroll
        for (int c = 0; c < R / 8; ++c) w[c] = bp[(int64_t)c * p.N];
        float wf[R];                                                                     // the column's r factors, unpacked once for all its rows
#pragma unroll
        for (int c = 0; c < R / 8; ++c) {
#pragma unroll
            for (int h = 0; h < 4; ++h) { wf[c * 8 + 2 * h] = lo_bf(w[c][h]); wf[c * 8 + 2 * h + 1] = hi_bf(w[c][h]); }
        }
        for (unsigned m = (unsigned)used_rows[k]; m != 0; m &= m - 1) {                  // the slot's rows, ascending
            const int i = __ffs(m) - 1;
            const f32x4* t = (const f32x4*)(ts + i * Rs + off);                          // (Rs and off are multiples of 16 floats)
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < R / 4; ++q) {
                const f32x4 tv = t[q];
                acc = fmaf(tv[0], wf[4 * q], acc); acc = fmaf(tv[1], wf[4 * q + 1], acc);
                acc = fmaf(tv[2], wf[4 * q + 2], acc); acc = fmaf(tv[3], wf[4 * q + 3], acc);
            }
            p.D[(int64_t)i * p.ldd + col] = acc;
        }
    }
}

int launch_lora_expand(const float* T, int64_t ldt, int n, const bf16_t* B, int64_t slot_stride, const int32_t* row_adapter, int capacity, float* D, int64_t ldd,
                       int N, int r, int c1, int c2, hipStream_t s) {
    VILA_REQUIRE(T != nullptr && B != nullptr && row_adapter != nullptr && D != nullptr, "lora expand: NULL argument");
    VILA_REQUIRE(n >= 1 && n <= 16, "lora expand: 1..16 sequences (got %d)", n);
    VILA_REQUIRE(capacity >= 1 && capacity <= LORA_MAX_SLOTS, "lora expand: 1..%d slots (got %d)", LORA_MAX_SLOTS, capacity);
    VILA_REQUIRE(r == 16 || r == 32 || r == 48 || r == 64, "lora expand: rank 16, 32, 48 or 64 (got %d)", r);
    VILA_REQUIRE(N > 0 && c1 >= 1 && c1 <= c2 && c2 <= N, "lora expand: segment ends 1 <= c1 (%d) <= c2 (%d) <= N (%d)", c1, c2, N);
    const int Rs = (1 + (c1 < N) + (c2 < N)) * r;
    VILA_REQUIRE(ldt >= Rs && ldd >= N && slot_stride >= (int64_t)r * N && slot_stride % 8 == 0 && (uintptr_t)B % 16 == 0,
                 "lora expand: operand alignment, or a stride shorter than what it spans");
    LoraExpandArgs a{T, ldt, B, slot_stride, row_adapter, D, ldd, n, N, c1, c2, capacity};
    const dim3 grid(cdiv(N, 256)), block(256);
    switch (r) {
        case 16: hipLaunchKernelGGL(lora_expand_kernel<16>, grid, block, 0, s, a); break;
        case 32: hipLaunchKernelGGL(lora_expand_kernel<32>, grid, block, 0, s, a); break;
        case 48: hipLaunchKernelGGL(lora_expand_kernel<48>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(lora_expand_kernel<64>, grid, block, 0, s, a); break;
    }
    VILA_LAUNCH_CHECK();
    return 0;
}

// ---- operator entries (include/vila_hip.h; tests/test_gpu_lora_serving_ops.py) ----------------------------------------------------------------------
extern "C" int vila_lora_shrink_bf16(const void* x, int64_t ldx, int n, const void* A, int64_t slot_stride, const float* scale, const int32_t* row_adapter,
                                     int capacity, float* T, int64_t ldt, int Rs, int K, vila_stream_t stream) {
    return launch_lora_shrink((const bf16_t*)x, ldx, n, (const bf16_t*)A, slot_stride, scale, row_adapter, capacity, T, ldt, Rs, K, vila_stream_enter((void*)stream));
}
extern "C" int vila_lora_expand_f32(const float* T, int64_t ldt, int n, const void* B, int64_t slot_stride, const int32_t* row_adapter, int capacity, float* D,
                                    int64_t ldd, int N, int r, int c1, int c2, vila_stream_t stream) {
    return launch_lora_expand(T, ldt, n, (const bf16_t*)B, slot_stride, row_adapter, capacity, D, ldd, N, r, c1, c2, vila_stream_enter((void*)stream));
}
